"""GPU: Localizer(mode="map") with MapConfig.keyframes -- a frame that the relocalisation grid leaves lost is compared
with the keyframes of the map and tracked once more from the best-scoring pose around the most similar ones -- at
160x120, "ED", in the box room of gsplatloc_amd.synthetic seen from POSITION, off the room's centre (from the centre the
box is symmetric, and two views half a turn apart are the same image).

(b) Real kernels, a stand-in tracker.  normalize=False, motion="hold", depth_rho 0.01, reloc_trans 0.1 m, a capacity of
    8 W H rows.  The map is grown from six frames at yaw 0, 60, .. 300 degrees about y from POSITION, tracked by a
    stand-in whose run() answers the frame's ground truth: each is accepted and each becomes a keyframe.  Then the
    stand-in answers its start pose, and the kidnapped frame comes: its pose is keyframe 2's turned by the one-cell yaw
    (place_base(.., 1, 0), 7.1 degrees) and moved by one reloc_trans step along the camera's x -- candidate 13 of the
    place grid, exactly.  The hold start (keyframe 5's pose) is rejected and the grid around it fails; match_place
    ranks keyframe 2 first with shift (1, 0), as the mirror on host copies does; the scored winner is candidate 13, the
    one the score mirror names; the frame ends lost=False, relocalised=True, recognised=2, eT == 0 and its rows go in at
    that pose.  The same frame with keyframes=False is lost and adds nothing: the test that fails without the feature.
    (depth_rho and reloc_trans: with the defaults, 0.05 and 0.05 m, the base and the exact candidate 5 cm beside it
    agree with the same rows and the tie goes to the base; a step of 0.3 m as in tests/test_gpu_map_reloc_localizer.py
    slides the image by a cell and the frame matches under (-1, 0).  Found with the two mirrors on the CPU, on the union
    of the six frames' back-projections: keyframe 2 first under (1, 0) with sum / common 122.3 against 420.6 for
    the runner-up, keyframe 0; candidate 13 with agree - front 29 907 against 886.)
(c) The turn from a shift, on the device: one room frame at P (yaw 120) is the only keyframe; queries at P @ R_y(-a) for
    sx in -2 .. 2 and P @ R_x(+b) for sy in -1 .. 1.  The best shift is (sx, 0), respectively (0, sy), and the base
    composed from it is nearer in rotation to the query's pose than P is.
(d) The real tracker, the settings and ITERS of tests/test_gpu_map_localizer.py.  A constant yaw of YAW_D degrees per
    frame about y from POSITION_D is tracked until the camera has turned 120 degrees; the next frame fed is frame
    BACK_TO again: the camera has been taken back.  With keyframes the frame is recognised and placed; without, it is
    lost.  In this room that is not so from every position: see the test's docstring.
(e) evaluate_room(..., map_reloc=True, map_keyframes=True) on the static 6-frame twist: recognised_frames == 0,
    keyframes >= 1; a plain report has neither key.

Measured on the MI355X: see the docstrings of the tests and NOTES.md, "Place recognition"."""
import numpy as np
import pytest
import torch

from gsplatloc_amd.localizer import Localizer, _step, place_base, reloc_candidates
from gsplatloc_amd.mapping import GaussianMap, MapConfig
from gsplatloc_amd.my_gsplat import TrackerConfig
from gsplatloc_amd.my_gsplat.trainer import TrackResult
from gsplatloc_amd.synthetic import replica_intrinsics, room_depth, write_replica_constant_twist
from tests import map_place_ref as ref
from tests import map_score_ref as score_ref
from tests.pose_ref import axis_angle
from tests.test_gpu_map_localizer import ITERS, N_B, H, W, _yardstick

pytestmark = pytest.mark.gpu
F32 = np.float32
POSITION = (0.6, 0.1, 0.8)
RHO_B, TRANS_B = 0.01, 0.1
POSITION_D = (-0.9, 0.2, 1.0)
YAW_D, N_D, BACK_TO = 6.0, 21, 2  # (d): frames 0 .. 20 turn 120 degrees; then frame 2 again


def _pose(yaw_deg, position=POSITION):
    c2w = torch.eye(4)
    c2w[:3, :3] = axis_angle((0.0, 1.0, 0.0), yaw_deg).float()
    c2w[:3, 3] = torch.tensor(position)
    return c2w


def _angle_between(a, b):
    R = a[:3, :3].double().T @ b[:3, :3].double()
    return float(np.degrees(np.arccos(np.clip((float(R.trace()) - 1.0) / 2.0, -1.0, 1.0))))


class _Tracker:
    """Stands in for GraphTracker: run() answers the reference pose of load_frame (the frame's ground truth) while
    ``truth`` is set, and the pose it was started from afterwards."""
    made, truth = [], True

    def __init__(self, N, W_, H_, config, device, render_mode):
        self.N, self.starts, self.refs = N, [], []
        _Tracker.made.append(self)

    def load_frame(self, tar_points, colors, scales, src_depth, tar_c2w, src_c2w, K, pixels=None):
        assert tar_points.shape == (self.N, 3)
        self.starts.append(tar_c2w.clone())
        self.refs.append(src_c2w.clone())

    def run(self):
        answer = self.refs[-1] if _Tracker.truth else self.starts[-1]
        return TrackResult(best_loss=0.25, steps=12, final_c2w=answer.clone(), best_c2w=answer.clone(), best_step=7)


def _grow(K, frames, poses, cfg):
    _Tracker.made, _Tracker.truth = [], True
    loc = Localizer(K, W, H, TrackerConfig(max_steps=ITERS), normalize=False, motion="hold", tracker_factory=_Tracker,
                    mode="map", map_config=cfg)
    loc.reset(*frames[0], poses[0])
    results = [loc.track(*f, gt_c2w=p) for f, p in zip(frames[1:], poses[1:])]
    _Tracker.made, _Tracker.truth = [], False
    return loc, results


def test_a_kidnapped_frame_is_recognised_and_placed_at_the_exact_candidate(capsys):
    """Measured on the MI355X: the map has 76 285 rows and six keyframes.  The hold start scores (tested, agree, front) =
    (19452, 265, 4539), share 0.0552, and its grid's winner, candidate 10, (18970, 276, 4203), share 0.0616.  The match:
    keyframe 2 under (1, 0) with sum / common 122.3, then keyframe 0 with 420.6, 1 with 589.5, 5 with 808.4, 3 with
    1042.3, 4 with 1126.2; keyframe 2's next shifts (1, -1) 131.3 and (1, 1) 133.9.  The place grid's winner is candidate
    13 with (18165, 18164, 0), the runner-up's agree - front is 526; 265 rows added.  Without keyframes the frame is lost
    0.100 m and 176.9 degrees from its pose."""
    K = replica_intrinsics(W, H)
    fx, fy = float(K[0, 0]), float(K[1, 1])
    intr = tuple(float(F32(a)) for a in (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))
    cfg = MapConfig(reloc=True, keyframes=True, depth_rho=RHO_B, reloc_trans=TRANS_B, capacity=8 * W * H)
    poses = [_pose(60.0 * k) for k in range(6)]
    gen = torch.Generator().manual_seed(5)
    image = lambda: torch.randint(0, 255, (H, W, 3), generator=gen).float()  # noqa: E731
    frames = [(room_depth(W, H, K, p), image()) for p in poses]
    exact = 1 + 6 * cfg.reloc_levels  # the first shift of a base's grid: +1 x reloc_trans along x
    base = place_base(poses[2], 1, 0, W, H, fx, fy)
    kid = reloc_candidates([base], cfg.reloc_rot_deg, cfg.reloc_trans, cfg.reloc_levels)[exact]
    assert abs(float((torch.linalg.inv(base.double()) @ kid.double())[0, 3]) - TRANS_B) < 1e-6
    assert abs(_angle_between(poses[2], kid) - np.degrees(np.arctan((W / 16.0) / fx))) < 1e-3
    kid_frame = (room_depth(W, H, K, kid), image())
    tcfg = TrackerConfig(max_steps=ITERS)
    near = tcfg.gs.near_plane

    loc, grown = _grow(K, frames, poses, cfg)
    assert [(r.lost, r.relocalised, r.recognised, r.keyframe) for r in grown] == [(False, False, -1, k) for k in range(1, 6)]
    assert loc.map.n_keyframes == 6 and not loc.map.full
    assert all(torch.equal(a, b) for a, b in zip(loc.map.keyframe_poses, poses))
    n0 = loc.map.n_live
    rows = loc.map.points.cpu().numpy().copy()
    score = lambda ps: score_ref.score(rows, np.stack([score_ref.w2c_of(p.numpy()) for p in ps]), intr,  # noqa: E731
                                       kid_frame[0].numpy(), F32(loc.map.keep), F32(loc.map.beyond), near)
    share = lambda c: c[1] / max(c[1] + c[2], 1)  # noqa: E731
    # the mirrors on host copies of the map as it is when the frame comes: the hold start and its grid
    grid1 = reloc_candidates([poses[5]], cfg.reloc_rot_deg, cfg.reloc_trans, cfg.reloc_levels)
    s1 = score(list(grid1))
    m1 = (s1[:, 1] - s1[:, 2]).tolist()
    w1 = m1.index(max(m1))
    # ... the match: the device's table and ranking against the mirror's
    table = np.stack([ref.describe(f[0].numpy()) for f in frames])
    assert np.array_equal(loc.map._place["table"][:6].cpu().numpy(), table)
    result = ref.match(ref.describe(kid_frame[0].numpy()), table)
    ranked = ref.rank(result, cfg.place_min_common)
    per_cell = [(r[0], r[1], r[2], round(r[3] / r[4], 1)) for r in ranked]
    own = sorted((t / c, ref.SHIFTS[s]) for s, (c, t) in enumerate(result[2].tolist()) if c >= cfg.place_min_common)
    # ... and the place grid
    bases = [place_base(poses[r[0]], r[1], r[2], W, H, fx, fy) for r in ranked[:cfg.place_top]]
    grid2 = reloc_candidates(bases, cfg.reloc_rot_deg, cfg.reloc_trans, cfg.reloc_levels)
    s2 = score(list(grid2))
    m2 = (s2[:, 1] - s2[:, 2]).tolist()
    w2 = m2.index(max(m2))
    with capsys.disabled():
        print(f"[place] (b) map rows {n0}; hold start (tested, agree, front) {s1[0].tolist()} share {share(s1[0]):.4f}; "
              f"its grid's winner {w1} {s1[w1].tolist()} share {share(s1[w1]):.4f}")
        print(f"[place] (b) match (slot, sx, sy, sum / common) {per_cell}; keyframe 2's shifts, best first "
              f"{[(s, round(v, 1)) for v, s in own[:3]]}")
        print(f"[place] (b) place grid winner {w2} {s2[w2].tolist()}, agree - front {m2[w2]} against the runner-up's "
              f"{sorted(m2)[-2]}")
    assert share(s1[0]) < cfg.reloc_min_agree and s1[0, 0] >= (W * H) // 16  # the hold start is rejected
    assert w1 == 0 or share(s1[w1]) < cfg.reloc_min_agree  # ... and its grid fails
    assert ranked[0][:3] == (2, 1, 0) and loc.map.match_place(kid_frame[0]) == ranked
    assert torch.equal(bases[0], base) and w2 == exact and torch.equal(grid2[w2], kid) and m2[w2] > sorted(m2)[-2]

    r = loc.track(*kid_frame, gt_c2w=kid)
    starts = [s.cpu() for t in _Tracker.made for s in t.starts]
    want_starts = [poses[5]] + ([grid1[w1]] if w1 != 0 else []) + [kid]
    assert len(starts) == len(want_starts) and all(torch.equal(a, b) for a, b in zip(starts, want_starts))
    assert (r.lost, r.relocalised, r.recognised, r.steps) == (False, True, 2, 12 * len(want_starts))
    assert torch.equal(r.c2w.cpu(), kid) and r.eT == 0.0
    assert (r.tested, r.agree, r.front) == tuple(s2[w2].tolist()) and r.front == 0
    # its rows went in at that pose: from there every one of them sits on the surface its own pixel observes
    assert r.added > 0 and r.map_size == n0 + r.added == loc.map.n_live
    new = loc.map.points[n0:].cpu().numpy()
    at = score_ref.score(new, score_ref.w2c_of(kid.numpy())[None], intr, kid_frame[0].numpy(), F32(loc.map.keep),
                         F32(loc.map.beyond), near)[0]
    assert at.tolist() == [r.added, r.added, 0]
    assert np.array_equal(loc.map.points[:n0].cpu().numpy().view(np.uint32), rows.view(np.uint32))
    assert r.keyframe == 6 and loc.map.n_keyframes == 7  # 7.1 degrees and 0.1 m from keyframe 2

    # the same frame without the option: lost, and the map is left alone
    plain_cfg = MapConfig(reloc=True, depth_rho=RHO_B, reloc_trans=TRANS_B, capacity=8 * W * H)
    plain, grown = _grow(K, frames, poses, plain_cfg)
    assert [(r.lost, r.recognised, r.keyframe) for r in grown] == [(False, None, None)] * 5 and plain.map.n_live == n0
    p = plain.track(*kid_frame, gt_c2w=kid)
    with capsys.disabled():
        print(f"[place] (b) added {r.added}; without keyframes: lost {p.lost}, (tested, agree, front) "
              f"{(p.tested, p.agree, p.front)}, eT {p.eT:.3f} m, eR {p.eR:.1f} degrees")
    assert (p.lost, p.relocalised, p.recognised, p.added) == (True, False, None, 0) and plain.map.n_live == n0
    assert np.array_equal(plain.map.points.cpu().numpy().view(np.uint32), rows.view(np.uint32))


def test_a_turned_camera_matches_under_the_shift_that_place_base_undoes_on_the_device(capsys):
    """Measured on the MI355X, sum / common of the best shift: 180.4, 97.6, 0.0, 115.2, 247.5 for sx = -2 .. 2 and 46.8,
    48.3 for sy = -1, 1; the base composed from it is 0.000 .. 0.023 degrees from the query's pose (float32), which was
    14.04, 7.13 and 5.40 degrees from the keyframe's.  The pose is one where the mirror finds all seven shifts; over 36
    poses of this room it finds a one-cell yaw exactly in 54 of 72 queries (NOTES.md, "Place recognition")."""
    K = replica_intrinsics(W, H)
    fx, fy = float(K[0, 0]), float(K[1, 1])
    P = _pose(120.0)
    m = GaussianMap(W, H, MapConfig(reloc=True, keyframes=True))
    assert m.add_keyframe(room_depth(W, H, K, P), P) == 0
    lines = []
    for sx, sy in [(s, 0) for s in range(-2, 3)] + [(0, -1), (0, 1)]:
        a, b = np.degrees(np.arctan(sx * (W / 16.0) / fx)), np.degrees(np.arctan(sy * (H / 12.0) / fy))
        Q = (P.double() @ _step(1, rot_deg=-a) @ _step(0, rot_deg=b)).float()
        depth = room_depth(W, H, K, Q)
        ranked = m.match_place(depth)
        assert ranked == ref.rank(ref.match(ref.describe(depth.numpy()), m._place["table"][:1].cpu().numpy()), 48)
        assert ranked[0][:3] == (0, sx, sy), (sx, sy, ranked)
        found = place_base(m.keyframe_poses[0], ranked[0][1], ranked[0][2], W, H, fx, fy)
        lines.append(f"({sx}, {sy}): {ranked[0][3] / ranked[0][4]:.1f}, {_angle_between(P, Q):.2f} -> "
                     f"{_angle_between(found, Q):.3f} degrees")
        assert _angle_between(found, Q) < 0.05 and (sx == sy == 0 or _angle_between(found, Q) < _angle_between(P, Q))
    with capsys.disabled():
        print("[place] (c) shift: sum / common, rotation to the query before -> after: " + "; ".join(lines))


def _run_back(root, map_config):
    """Localizer(mode="map") over frames 0 .. N_D - 1 of the sequence and then frame BACK_TO again."""
    from gsplatloc_amd.data import Parser

    parser = Parser("Replica", "room0", normalize=True, input_folder=str(root))
    depth, rgb, pose = parser.frame(0)
    loc = Localizer(parser.K, W, H, TrackerConfig(max_steps=ITERS), mode="map", map_config=map_config)
    loc.reset(depth, rgb, pose)
    gts, results = [pose], []
    for i in list(range(1, N_D)) + [BACK_TO]:
        depth, rgb, pose = parser.frame(i)
        results.append(loc.track(depth, rgb, gt_c2w=pose))
        gts.append(pose)
    return dict(traj=loc.trajectory, gts=torch.stack(gts), results=results, loc=loc, depth=depth)


def _share(r):
    return r.agree / (r.agree + r.front) if r.agree + r.front > 0 else None


def _bits(run, n):
    return (run["traj"][:n].cpu().numpy().view(np.uint32), [r.steps for r in run["results"][:n - 1]],
            [r.added for r in run["results"][:n - 1]])


def test_a_camera_taken_back_is_recognised_by_the_real_tracker(tmp_path, capsys):
    """Frames 0 .. 20 of a constant yaw of 6 degrees about y from POSITION_D, then frame 2 again: the constant-velocity
    start of that frame is 114 degrees from its pose.  With keyframes: nothing before the jump is lost or relocalised, and
    poses, steps and added rows before the jump are those of the run without keyframes -- bit for bit where two runs
    without the option repeat bit for bit, else within their difference, as tests/test_gpu_map_reloc_localizer.py does
    it; the jump frame is relocalised, recognised, and its absolute translation error is under twice the sum of the
    yardstick's pair errors.  Without: the jump frame is lost.

    Measured on the MI355X, a sweep of 4 positions x (6 degrees x 20 or 22, 7.5 degrees x 16 or 17) x (back to frame 0
    or 2): in 19 of 32 cases the jump frame was recognised with eT 0.000 .. 0.130 m and was lost without the option.  In
    all 8 cases from (0.6, 0.1, 0.8) the FIRST run's estimate, a quarter turn and 0.35 .. 0.96 m from the truth, was
    accepted with and without the option alike, e.g. (tested, agree, front) = (23213, 20773, 0): a box seen from inside
    has, for a view of two walls, the floor and the ceiling, an exact alias a quarter turn on, and the map is that box.
    The rule of MapConfig.reloc cannot tell them apart and place recognition is never asked; the same happened in the
    other 5 cases, with a wrong estimate accepted from the first or the second run.  This case, (-0.9, 0.2, 1.0),
    6 degrees x 20, back to 2: with keyframes relocalised from keyframe 2 with eT 0.038 m, 4304 steps in three runs,
    (21342, 21342, 0), under the bound of 0.246 m; without: lost, eT 0.676 m, eR 120.6 degrees, (2802, 1052, 823); two runs
    without the option repeated bit for bit before the jump, and the run with keyframes gave the same bits.  NOTES.md, "Place recognition"."""
    write_replica_constant_twist(tmp_path, W, H, N_D, rot_deg=YAW_D, trans=0.0, axis=(0.0, 1.0, 0.0),
                                 start=_pose(0.0, POSITION_D).numpy())
    bound = 2.0 * sum(_yardstick(tmp_path, N_D))
    capacity = 8 * W * H
    plain, again = (_run_back(tmp_path, MapConfig(reloc=True, capacity=capacity)) for _ in range(2))
    with_kf = _run_back(tmp_path, MapConfig(reloc=True, keyframes=True, capacity=capacity))
    res, pres = with_kf["results"], plain["results"]
    jump, pjump = res[-1], pres[-1]
    err = (with_kf["traj"][:, :3, 3] - with_kf["gts"][:, :3, 3]).norm(dim=1).tolist()
    (p1, s1, a1), (p2, s2, a2), (pk, sk, ak) = _bits(plain, N_D), _bits(again, N_D), _bits(with_kf, N_D)
    repeats = np.array_equal(p1, p2) and s1 == s2 and a1 == a2
    diff = lambda x, y: float(np.abs(x.view(np.float32) - y.view(np.float32)).max())  # noqa: E731
    gap = lambda x, y: max(abs(a - b) for a, b in zip(x, y))  # noqa: E731
    with capsys.disabled():
        print(f"[place] (d) {YAW_D} degrees x {N_D - 1}, then frame {BACK_TO} again; bound 2 sum eT_i {bound:.3e} m; two "
              f"runs without keyframes repeat bit for bit before the jump: {repeats}")
        print(f"[place] (d) with keyframes: steps {[r.steps for r in res]}, keyframe {[r.keyframe for r in res]}, share "
              f"{['%.4f' % _share(r) if _share(r) is not None else None for r in res]}, abs error "
              f"{['%.2e' % e for e in err[1:]]}")
        print(f"[place] (d) jump frame with keyframes: lost {jump.lost} relocalised {jump.relocalised} recognised "
              f"{jump.recognised} (tested, agree, front) {(jump.tested, jump.agree, jump.front)} eT {jump.eT:.3e} eR "
              f"{jump.eR:.3e} steps {jump.steps}; without: lost {pjump.lost} relocalised {pjump.relocalised} "
              f"{(pjump.tested, pjump.agree, pjump.front)} eT {pjump.eT:.3e} eR {pjump.eR:.3e} steps {pjump.steps}")
        print(f"[place] (d) match table of the jump frame {with_kf['loc'].map.match_place(with_kf['depth'])[:4]}; "
              f"keyframes {with_kf['loc'].map.n_keyframes}")
    # before the jump: nothing lost or relocalised, and the bits of the run without keyframes
    assert not any(r.lost or r.relocalised for r in res[:-1]) and not any(r.lost or r.relocalised for r in pres[:-1])
    assert all(r.recognised == -1 for r in res[:-1]) and all(r.recognised is None for r in pres)
    if repeats:
        assert np.array_equal(pk, p1) and sk == s1 and ak == a1
    else:
        assert diff(pk, p1) <= diff(p2, p1) and gap(sk, s1) <= gap(s2, s1) and gap(ak, a1) <= gap(a2, a1)
    # the jump frame
    assert not jump.lost and jump.relocalised and jump.recognised >= 0
    assert jump.eT < bound, (jump.eT, bound)
    assert pjump.lost and pjump.added == 0 and pjump.recognised is None


def test_the_evaluation_driver_reports_keyframes(tmp_path):
    from gsplatloc_amd.data import Parser
    from gsplatloc_amd.eval import evaluate_room

    write_replica_constant_twist(tmp_path, W, H, N_B, rot_deg=0.4, trans=0.01)
    parser = Parser("Replica", "room0", normalize=True, input_folder=str(tmp_path))
    r = evaluate_room(parser, ITERS, None, sequential=True, map_mode=True, map_reloc=True, map_keyframes=True)
    assert r["recognised_frames"] == 0 and r["keyframes"] >= 1 and r["lost_frames"] == 0 and r["relocalised_frames"] == 0
    plain = evaluate_room(parser, ITERS, None, sequential=True, map_mode=True, map_reloc=True)
    assert "recognised_frames" not in plain and "keyframes" not in plain
