"""Covisibility and the loops closed in track() (csrc/map_covis.hip, GaussianMap.covisibility, Localizer.add_loop and
MapConfig.loop), the parts that need no GPU: the mirror tests/map_covis_ref.py clause by clause, the pinned integers of
the room loop, ``GaussianMap.covisibility`` on a map whose device calls are the mirrors, the policy of ``track()`` around
stand-ins with every status reached by a scripted frame, the entry point's argument checks and the kernel's registers.

The room loop (tests/map_correct_ref.room_loop): eight 160 x 120 frames of the box room, every one inserted whole at its
drifted pose (0.3 degrees and 5 mm a frame).  From the drifted pose of frame 7 the rows of frame 0 are all tested and 657
of them lie in FRONT of what frame 7 sees -- the drift shows as rows seen through; from its true pose none do.

The policy runs on the 32 x 24 sequence of tests/test_map_cpu.py: the stand-in tracker answers the pose it is handed as
ground truth, so a drifted ``gt_c2w`` scripts the estimate, and the map's alignment is scripted per frame (its status and
its pose); the covisibility and the scores are the mirrors on the map's real rows."""
import ctypes
import os

import numpy as np
import pytest
import torch

from gsplatloc_amd import _lib
from gsplatloc_amd.localizer import LOOP_STATUS, Localizer, TrajectoryCorrection
from gsplatloc_amd.mapping import ALIGN_STATUS, GaussianMap, MapConfig, PoseGraphResult
from gsplatloc_amd.my_gsplat import TrackerConfig
from gsplatloc_amd.synthetic import room_depth
from tests import map_correct_ref
from tests import map_covis_ref as ref
from tests import map_score_ref
from tests import test_map_correct_cpu as cpu
from tests import test_map_cpu as base
from tests import test_map_refine_cpu as refine_cpu
from tests.map_score_ref import beyond_of, keep_of
from tests.test_abi import prototypes
from tests.test_kernel_resources import HIPCC, _resources
from tests.test_map_cpu import sequence  # noqa: F401  (the 32x24 drifting sequence, a module fixture there)

F32 = np.float32
EYE = np.eye(4, dtype=F32)
INTR = (50.0, 40.0, 15.5, 11.5)
KEEP, BEYOND = keep_of(0.25), beyond_of(0.25)
FLAT = np.full((24, 32), 2.0, F32)


def _p(u, v, z):
    """The point that projects onto pixel (u, v) at the depth z from the identity pose."""
    return [(u - INTR[2]) / INTR[0] * z, (v - INTR[3]) / INTR[1] * z, z]


def _covis(points, origins, n_frames, depth=FLAT, w2c=EYE, near=0.25):
    return ref.covis(np.asarray(points, F32), np.asarray(origins, np.int32), w2c, INTR, depth, KEEP, BEYOND, near,
                     n_frames)


# ---- the mirror, clause by clause -----------------------------------------------------------------------------------
def test_the_three_verdicts_are_binned_by_origin():
    points = [_p(3, 4, 2.0), _p(5, 4, 1.0), _p(7, 4, 3.0), _p(9, 4, 2.0), _p(11, 4, 1.0)]
    counts, outside = _covis(points, [0, 0, 2, 2, 2], 3)
    # frame 0: one row on the surface, one in front; frame 1: nothing; frame 2: one behind, one on, one in front
    assert counts.tolist() == [[2, 1, 1], [0, 0, 0], [3, 1, 1]] and outside == 0
    assert counts.dtype == np.int64 and counts.shape == (3, 3)
    # the order of the rows is not looked at
    perm = [4, 0, 3, 1, 2]
    again, _ = _covis([points[j] for j in perm], [[0, 0, 2, 2, 2][j] for j in perm], 3)
    assert np.array_equal(again, counts)


def test_the_origin_is_looked_at_first():
    nan = [np.nan, np.nan, np.nan]
    counts, outside = _covis([_p(3, 4, 2.0), nan, _p(3, 4, 2.0), nan, _p(5, 5, 2.0)], [-1, 7, 3, -2 ** 31, 2], 3)
    # a NaN row outside the table counts as outside, and so does a good row; neither is tested
    assert outside == 4 and counts.tolist() == [[0, 0, 0], [0, 0, 0], [1, 1, 0]]
    counts, outside = _covis([nan, [np.inf, 0.0, 2.0], _p(3, 4, -2.0)], [0, 1, 1], 2)
    assert outside == 0 and not counts.any()  # inside the table: not a number, not in front of the camera -- nothing


def test_the_thresholds_agree():
    d = np.float32(2.0)
    lo, hi = d * KEEP, d * BEYOND
    below, above = np.nextafter(lo, F32(0)), np.nextafter(hi, F32(9))
    pts = [[0.0, 0.0, float(z)] for z in (lo, below, hi, above)]
    centre = (INTR[0], INTR[1], 16.0, 12.0)  # x = y = 0 lands on pixel (16, 12) whatever z is
    counts, _ = ref.covis(np.asarray(pts, F32), np.arange(4, dtype=np.int32), EYE, centre, FLAT, KEEP, BEYOND, 0.25, 4)
    # z == d * keep agrees, the float below it is in front; z == d * beyond agrees, the float above it is behind
    assert counts.tolist() == [[1, 1, 0], [1, 0, 1], [1, 1, 0], [1, 0, 0]]


def test_pixels_without_depth_and_the_image_border():
    depth = FLAT.copy()
    depth[4, 3], depth[4, 5], depth[4, 7], depth[4, 9] = 0.0, np.nan, np.inf, -1.0
    pts = [_p(u, 4, 2.0) for u in (3, 5, 7, 9, 11)] + [_p(-0.5, 4, 2.0), _p(-0.51, 4, 2.0), _p(31.49, 4, 2.0), _p(31.51, 4, 2.0),
                                                      _p(5, -0.5, 2.0), _p(5, 23.51, 2.0)]
    counts, outside = _covis(pts, list(range(11)), 11, depth)
    assert outside == 0
    assert counts[:, 0].tolist() == [0, 0, 0, 0, 1, 1, 0, 1, 0, 1, 0]  # rint(-0.5) = -0 is column / line 0
    # the near plane: z > near, not >=
    counts, _ = _covis([_p(3, 4, 2.0)] * 2, [0, 1], 2, near=2.0)
    assert not counts.any()


def test_a_negative_zero():
    pts = np.array([[-0.0, -0.0, 2.0]], F32)
    centre = (INTR[0], INTR[1], 16.0, 12.0)
    a, _ = ref.covis(pts, [0], EYE, centre, FLAT, KEEP, BEYOND, 0.25, 1)
    b, _ = ref.covis(np.abs(pts), [0], EYE, centre, FLAT, KEEP, BEYOND, 0.25, 1)
    assert a.tolist() == b.tolist() == [[1, 1, 0]]
    neg = np.where(EYE == 0, F32(-0.0), EYE)  # -0.0 for the zeros of the pose
    c, _ = ref.covis(np.abs(pts), [0], neg, centre, FLAT, KEEP, BEYOND, 0.25, 1)
    assert c.tolist() == [[1, 1, 0]]


def test_the_sum_over_the_frames_is_the_score():
    rng = np.random.default_rng(5)
    pts = rng.uniform(-0.4, 0.4, (4000, 3)).astype(F32)
    pts[:, 2] = rng.uniform(0.1, 4.0, 4000)
    pts[:, :2] *= pts[:, 2:]  # a little wider than the image
    pts[::97] = np.nan
    depth = rng.uniform(1.0, 3.0, (24, 32)).astype(F32)
    depth[rng.random((24, 32)) < 0.15] = 0.0
    w2c = np.linalg.inv(map_correct_ref.twist(4.0, 0.1)).astype(F32)
    origins = rng.integers(0, 9, 4000).astype(np.int32)  # shuffled: the order of the origins is not looked at
    counts, outside = ref.covis(pts, origins, w2c, INTR, depth, KEEP, BEYOND, 0.25, 9)
    want = map_score_ref.score(pts, w2c[None], INTR, depth, KEEP, BEYOND, 0.25)[0]
    assert outside == 0 and counts.sum(axis=0).tolist() == want.tolist() and want[0] > 500 and want[2] > 50
    # a table that is too short: the rows behind it are outside, the others keep their counts
    short, outside = ref.covis(pts, origins, w2c, INTR, depth, KEEP, BEYOND, 0.25, 6)
    assert np.array_equal(short, counts[:6]) and outside == int((origins >= 6).sum())


# ---- the room loop: pinned integers ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def room():
    return ref.room_loop_map()


@pytest.mark.parametrize("pose", ["drifted", "true"])
def test_the_room_loop_from_frame_seven(room, pose):
    rows, origins, true, est, depths, intr, _ = room
    n = 7 * 160 * 120  # the rows of frames 0 .. 6
    at = est[7] if pose == "drifted" else true[7]
    w2c = np.linalg.inv(at).astype(F32)
    near = TrackerConfig().gs.near_plane
    counts, outside = ref.covis(rows[:n], origins[:n], w2c, intr, depths[7], keep_of(0.05), beyond_of(0.05), near, 7)
    print(f"[covis] room loop, frame 7 at its {pose} pose: tested {counts[:, 0].tolist()} agree {counts[:, 1].tolist()} "
          f"front {counts[:, 2].tolist()}")
    assert outside == 0
    assert counts[:, 0].tolist() == ref.ROOM_TESTED[pose]
    assert counts[:, 2].tolist() == ref.ROOM_FRONT[pose]
    assert counts[:, 1].tolist() == ref.ROOM_AGREE[pose]
    if pose == "drifted":
        assert counts[0].tolist() == [19200, 18543, 657]  # what the prefix of frame 0 scores (NOTES.md)
    score = map_score_ref.score(rows[:n], w2c[None], intr, depths[7], keep_of(0.05), beyond_of(0.05), near)[0]
    assert counts.sum(axis=0).tolist() == score.tolist()


# ---- GaussianMap.covisibility on a map whose device calls are the mirrors ---------------------------------------------
W, H = base.W, base.H
K = cpu.K
NEAR = cpu.NEAR
CONVERGED, FEW, STEPPED = (ALIGN_STATUS.index(s) for s in ("CONVERGED", "FEW", "STEPPED"))


class _LoopMirrorMap(cpu._CorrectMirrorMap):
    """The mirror map of the correction tests; the covisibility and the scores are the mirrors on the prefix they are
    given, and the alignment answers what the test scripted: ``answers`` holds per call (status, steps applied, the
    aligned camera-to-world pose or None for the start)."""
    answers = []

    def _rows(self, n_rows):
        return self.n_live if n_rows is None else n_rows

    def _covis_launch(self, depth, intr, w2c, near, n_frames, n_rows=None):
        n = self._rows(n_rows)
        assert w2c.dtype == torch.float32 and w2c.shape == (4, 4) and w2c.is_contiguous()
        self._say("covis", n_frames=n_frames, n_rows=n_rows, w2c=w2c.numpy().copy())
        return ref.covis(self.means[:n].numpy(), self.origins[:n].numpy(), w2c.numpy(), intr, depth.numpy(),
                         F32(self.keep), F32(self.beyond), near, n_frames)

    def _score_launch(self, depth, intr, w2c, near, n_rows=None):
        n = self._rows(n_rows)
        self._say("score", n_rows=n_rows)
        return map_score_ref.score(self.means[:n].numpy(), w2c.numpy(), intr, depth.numpy(), F32(self.keep),
                                   F32(self.beyond), near)

    def _align_launch(self, depth, intr, w2c, *args, n_rows=None):
        status, steps, c2w = type(self).answers.pop(0)
        self._say("align", n_rows=n_rows)
        pose = w2c.numpy().astype(np.float64) if c2w is None else np.linalg.inv(np.asarray(c2w, np.float64))
        return pose[:3], pose.astype(F32), steps, np.array([[status, 50, 60, 0]], np.int64), np.zeros((1, 6))


def _filled(config=None):
    """A map of the 32 x 24 room: frame 0 whole, frames 1, 2 and 5 one image column each."""
    m = _LoopMirrorMap(W, H, config or MapConfig(origins=True, capacity=W * H + 4 * H), "cpu")
    depth, rgb = room_depth(W, H, K, torch.eye(4)), torch.full((H, W, 3), 100.0)
    render, alphas = torch.full((H, W), 0.01), torch.ones(H, W)
    alphas[:, 0] = 0.25
    m.insert_frame(depth, rgb, K, torch.eye(4), origin=0)
    for k in (1, 2, 5):
        m.insert_frame(depth, rgb, K, torch.eye(4), render, alphas, origin=k)
    return m, depth


def test_covisibility_of_a_map():
    m, depth = _filled()
    refine_cpu._RefineMirrorMap.log = []
    c = m.covisibility(depth, K, torch.eye(4), NEAR)
    call = refine_cpu._RefineMirrorMap.log[-1]
    assert call["call"] == "covis" and call["n_frames"] == 6 and call["n_rows"] is None  # the last origin written + 1
    assert c.dtype == np.int64 and c.shape == (6, 3) and m.last_covis_outside == 0
    assert c[:, 0].tolist() == [W * H, H, H, 0, 0, H] and np.array_equal(c[:, 0], c[:, 1]) and not c[:, 2].any()
    assert c.sum(axis=0).tolist() == m.score_poses(depth, K, [torch.eye(4)], NEAR)[0].tolist()
    # keep and beyond are the map's own
    assert np.array_equal(call["w2c"], np.eye(4, dtype=F32))
    # a table that ends before the last frame: its rows are outside, and reported
    c3 = m.covisibility(depth, K, torch.eye(4), NEAR, n_frames=3)
    assert np.array_equal(c3, c[:3]) and m.last_covis_outside == H
    c9 = m.covisibility(depth, K, torch.eye(4), NEAR, n_frames=np.int64(9))
    assert np.array_equal(c9[:6], c) and not c9[6:].any() and m.last_covis_outside == 0
    # a prefix, as score_poses takes one
    rows = m.rows_up_to(1)
    cp = m.covisibility(depth, K, torch.eye(4), NEAR, rows=rows)
    assert refine_cpu._RefineMirrorMap.log[-1]["n_rows"] == rows
    assert cp[:, 0].tolist() == [W * H, H, 0, 0, 0, 0]
    assert cp.sum(axis=0).tolist() == m.score_poses(depth, K, [torch.eye(4)], NEAR, rows=rows)[0].tolist()
    # a pose that sees the room from 30 cm further back: rows are in front of nothing, the counts still add up
    back = torch.eye(4)
    back[2, 3] = -0.3
    cb = m.covisibility(depth, K, back, NEAR)
    assert cb.sum(axis=0).tolist() == m.score_poses(depth, K, [back], NEAR)[0].tolist() and cb[0, 1] < cb[0, 0]
    # no rows: zeros, and nothing is launched
    calls = len(refine_cpu._RefineMirrorMap.log)
    assert not m.covisibility(depth, K, torch.eye(4), NEAR, rows=0).any()
    empty = _LoopMirrorMap(W, H, MapConfig(origins=True), "cpu")
    z = empty.covisibility(depth, K, torch.eye(4), NEAR)
    assert z.shape == (1, 3) and not z.any() and len(refine_cpu._RefineMirrorMap.log) == calls
    for bad in (0, -1, 1.5, True, 2 ** 24 + 1):
        with pytest.raises(ValueError, match="n_frames"):
            m.covisibility(depth, K, torch.eye(4), NEAR, n_frames=bad)
    with pytest.raises(ValueError, match="rows"):
        m.covisibility(depth, K, torch.eye(4), NEAR, rows=m.n_live + 1)
    with pytest.raises(ValueError):
        m.covisibility(depth, K, torch.eye(3), NEAR)


def test_covisibility_needs_the_origins_and_a_device():
    m = _LoopMirrorMap(W, H, MapConfig(), "cpu")
    with pytest.raises(RuntimeError, match="origins"):
        m.covisibility(torch.full((H, W), 2.0), K, torch.eye(4), NEAR)
    host = GaussianMap(W, H, MapConfig(origins=True), "cpu")
    host.n_live = 3
    with pytest.raises(AssertionError, match="no CPU path"):
        host.covisibility(torch.full((H, W), 2.0), K, torch.eye(4), NEAR)


def test_map_config_validation():
    c = MapConfig()
    assert (c.loop, c.loop_min_gap, c.loop_every, c.loop_min_rows, c.loop_min_agree, c.loop_min_trans,
            c.loop_min_rot_deg, c.loop_weight, c.loop_by) == (False, 30, 10, None, 0.9, 0.005, 0.1, 1e4, "index")
    MapConfig(origins=True, loop=True, loop_min_gap=1, loop_every=1, loop_min_rows=1, loop_min_agree=1.0,
              loop_min_trans=0.0, loop_min_rot_deg=0.0, loop_weight=1, loop_by="path")
    with pytest.raises(ValueError, match="origins"):
        MapConfig(loop=True)
    for kw, word in ((dict(loop=1), "loop"), (dict(loop=None), "loop"), (dict(loop="yes"), "loop"),
                     (dict(loop_min_gap=0), "loop_min_gap"), (dict(loop_min_gap=1.5), "loop_min_gap"),
                     (dict(loop_every=0), "loop_every"), (dict(loop_every=True), "loop_every"),
                     (dict(loop_min_rows=0), "loop_min_rows"), (dict(loop_min_rows=2.5), "loop_min_rows"),
                     (dict(loop_min_agree=0.0), "loop_min_agree"), (dict(loop_min_agree=1.01), "loop_min_agree"),
                     (dict(loop_min_trans=-1e-3), "loop_min_trans"), (dict(loop_min_trans=float("nan")), "loop_min_trans"),
                     (dict(loop_min_rot_deg=float("inf")), "loop_min_rot_deg"), (dict(loop_weight=0.0), "loop_weight"),
                     (dict(loop_weight=float("inf")), "loop_weight"), (dict(loop_by="time"), "loop_by")):
        with pytest.raises(ValueError, match=word):
            MapConfig(origins=True, **kw)


# ---- the policy of track() around stand-ins ---------------------------------------------------------------------------
def _localizer(config, monkeypatch, answers=()):
    import gsplatloc_amd.data.dataset as DS

    monkeypatch.setattr(DS, "compute_depth_gt", lambda pts, col, Ks, c2w, height, width: torch.zeros(height, width))
    base._Tracker.made = []
    refine_cpu._RefineMirrorMap.log = []
    _LoopMirrorMap.answers = list(answers)
    return Localizer(K, W, H, TrackerConfig(max_steps=5), normalize=False, motion="hold", device="cpu",
                     tracker_factory=base._Tracker, mode="map", map_factory=_LoopMirrorMap,
                     map_renderer=refine_cpu._Renderer(), map_config=config)


def _shifted(pose, metres, axis=2):
    out = np.asarray(pose, np.float64).copy()
    out[:3, 3] += metres * out[:3, axis]
    return out


LOOP_FIELDS = ("loop", "loop_status", "loop_old_tested", "loop_anchor", "loop_moved_t", "loop_moved_r_deg",
               "loop_correction")


def test_every_status_short_of_a_closure_and_nothing_changes(sequence, monkeypatch):  # noqa: F811
    assert LOOP_STATUS == ("waiting", "few_rows", "not_converged", "rejected", "small", "closed")
    poses = [sequence[k][2].double().numpy() for k in range(base.N_FRAMES)]
    plain = _localizer(MapConfig(origins=True), monkeypatch)
    plain.reset(*sequence[0])
    plain_results = [plain.track(sequence[k][0], sequence[k][1], gt_c2w=sequence[k][2]) for k in range(1, base.N_FRAMES)]
    assert all(getattr(r, f) is None for r in plain_results for f in LOOP_FIELDS)
    assert not [c for c in refine_cpu._RefineMirrorMap.log if c["call"] in ("covis", "align")]
    plain_calls = [c["call"] for c in refine_cpu._RefineMirrorMap.log]

    cfg = MapConfig(origins=True, loop=True, loop_min_gap=2, loop_every=1, loop_min_rows=100)
    answers = [(FEW, 0, None),  # frame 2: the alignment refuses
               (CONVERGED, 2, _shifted(poses[3], 0.5)),  # frame 3: it settles half a metre off, where nothing agrees
               (CONVERGED, 1, _shifted(poses[4], 1e-4))]  # frame 4: it moves by a tenth of a millimetre
    loc = _localizer(cfg, monkeypatch, answers)
    loc.reset(*sequence[0])
    results = [loc.track(sequence[k][0], sequence[k][1], gt_c2w=sequence[k][2]) for k in range(1, base.N_FRAMES)]
    assert [r.loop_status for r in results] == ["few_rows", "not_converged", "rejected", "small"]
    assert all(r.loop is False and r.loop_anchor is None and r.loop_correction is None for r in results)
    assert results[0].loop_old_tested == 0 and all(r.loop_old_tested >= 100 for r in results[1:])
    assert results[2].loop_moved_t is None and abs(results[3].loop_moved_t - 1e-4) <= 2e-6
    assert _LoopMirrorMap.answers == [] and loc._loops == [] and loc.last_pose_graph is None
    # frame 1 has no frame two behind it: nothing is launched for it.  Frames 2 .. 4: one covisibility at the
    # estimate over frames 0 .. n - 1, then the constraint against the prefix of the frames up to n - 2 -- all of it
    # before the frame's insertion
    calls = [(c["call"], c.get("n_rows"), c.get("n_frames")) for c in refine_cpu._RefineMirrorMap.log]
    per_frame, cur = [], []
    for c in calls:
        cur.append(c)
        if c[0] == "insert":
            per_frame.append(cur)
            cur = []
    assert [[c[0] for c in f] for f in per_frame[1:]] == [["render", "insert"]] + [["covis", "align", "score", "render",
                                                                                  "insert"]] * 3
    assert [f[0][1:] for f in per_frame[2:]] == [(None, 2), (None, 3), (None, 4)]
    assert [f[1][1] for f in per_frame[2:]] == [W * H, W * H + H, W * H + 2 * H]  # rows_up_to(n - 2)
    assert [c for c in [x[0] for x in calls] if c not in ("covis", "align", "score")] == plain_calls
    # with no closure the trajectory and the map are those of the run without the option, bit for bit
    assert torch.equal(loc.trajectory, plain.trajectory) and loc.map.n_live == plain.map.n_live
    assert torch.equal(loc.map.points, plain.map.points) and torch.equal(loc.map.point_colors, plain.map.point_colors)
    assert torch.equal(loc.map.origins[:loc.map.n_live], plain.map.origins[:plain.map.n_live])
    for a, b in zip(results, plain_results):
        assert torch.equal(a.c2w, b.c2w) and (a.added, a.steps, a.map_size) == (b.added, b.steps, b.map_size)
    # the odometry is recorded with the origins, one measurement per appended pose, in float64
    assert len(loc._odometry) == len(plain._odometry) == base.N_FRAMES - 1
    T = loc.trajectory.double().numpy()
    for k, Z in enumerate(loc._odometry):
        assert Z.dtype == np.float64 and np.array_equal(Z, np.linalg.inv(T[k]) @ T[k + 1])
    loc.reset(*sequence[0])
    assert loc._odometry == [] and loc._loops == []


def test_waiting_and_few_rows(sequence, monkeypatch):  # noqa: F811
    cfg = MapConfig(origins=True, loop=True, loop_min_gap=1, loop_every=3, loop_min_rows=2 * W * H)
    loc = _localizer(cfg, monkeypatch)
    loc.reset(*sequence[0])
    results = [loc.track(sequence[k][0], sequence[k][1], gt_c2w=sequence[k][2]) for k in range(1, base.N_FRAMES)]
    # an attempt at frame 3 (three frames after the reset), which finds fewer old rows tested than it was told to ask for
    assert [r.loop_status for r in results] == ["waiting", "waiting", "few_rows", "waiting"]
    assert [r.loop_old_tested for r in results] == [None, None, results[2].loop_old_tested, None]
    assert 0 < results[2].loop_old_tested < 2 * W * H
    assert [c["call"] for c in refine_cpu._RefineMirrorMap.log].count("covis") == 1
    # without the origins the option is refused, and a lost frame is not asked
    with pytest.raises(ValueError, match="origins"):
        MapConfig(loop=True)
    loc = _localizer(MapConfig(origins=True, loop=True, loop_min_gap=1, loop_every=1), monkeypatch)
    loc.reset(*sequence[0])
    loc._factory = base._LostTracker
    r = loc.track(sequence[1][0], sequence[1][1])
    assert r.lost and r.loop is False and r.loop_status is None and len(loc._odometry) == 1
    assert not [c for c in refine_cpu._RefineMirrorMap.log if c["call"] == "covis"]


def test_a_closed_loop(sequence, monkeypatch):  # noqa: F811
    """The estimates drift by 1 cm a frame along the camera's x axis; at frame 3 the alignment against the rows of
    frames 0 and 1 answers the frame's true pose."""
    truth = [sequence[k][2].double().numpy() for k in range(base.N_FRAMES)]
    drift = [torch.from_numpy(_shifted(truth[k], 0.01 * k, axis=0)).float() for k in range(base.N_FRAMES)]
    cfg = MapConfig(origins=True, loop=True, loop_min_gap=2, loop_every=3, loop_min_rows=100)
    aligned = torch.from_numpy(truth[3]).float()
    loc = _localizer(cfg, monkeypatch, [(CONVERGED, 3, aligned.double().numpy())])
    loc.reset(*sequence[0])
    r1 = loc.track(sequence[1][0], sequence[1][1], gt_c2w=drift[1])
    r2 = loc.track(sequence[2][0], sequence[2][1], gt_c2w=drift[2])
    assert (r1.loop_status, r2.loop_status) == ("waiting", "waiting")
    old = loc.trajectory.double().numpy()
    rows_before, n_before = loc.map.points.clone(), loc.map.n_live
    assert n_before == W * H + 2 * H
    refine_cpu._RefineMirrorMap.log = []
    r = loc.track(sequence[3][0], sequence[3][1], gt_c2w=drift[3])
    assert r.loop is True and r.loop_status == "closed" and r.loop_anchor == 0
    assert r.loop_old_tested >= 100 and abs(r.loop_moved_t - 0.03) <= 1e-5 and r.loop_moved_r_deg <= 1e-3
    calls = [c["call"] for c in refine_cpu._RefineMirrorMap.log]
    # the covisibility at the estimate, the constraint, the covisibility at the aligned pose, the correction -- and
    # only then the frame's own insertion
    assert calls[:7] == ["covis", "align", "score", "covis", "correct", "render", "insert"]
    second = refine_cpu._RefineMirrorMap.log[3]
    assert np.array_equal(second["w2c"], np.linalg.inv(aligned.double().numpy()).astype(F32))
    # the anchor: the old frame with the most agreeing rows from the aligned pose
    intr = tuple(float(torch.as_tensor(K, dtype=torch.float32)[i, j]) for i, j in ((0, 0), (1, 1), (0, 2), (1, 2)))
    want = ref.covis(rows_before.numpy(), loc.map.origins[:n_before].numpy(), second["w2c"], intr,
                     sequence[3][0].numpy(), F32(loc.map.keep), F32(loc.map.beyond), NEAR, 3)[0]
    assert r.loop_anchor == int(np.argmax(want[:2, 1])) and want[0, 1] > want[1, 1] > 0
    # the pose graph: one edge from frame 0, frame 0 held; the corrected pose of frame 3 is the aligned one
    g = loc.last_pose_graph
    assert isinstance(g, PoseGraphResult) and g.converged and g.cost_after < g.cost_before
    assert len(loc._loops) == 1 and loc._loops[0][:2] == (0, 3) and loc._loops[0][3] == cfg.loop_weight
    assert np.abs(loc._loops[0][2] - np.linalg.inv(old[0]) @ aligned.double().numpy()).max() <= 1e-12
    assert g.loop_residuals.shape == (1,) and g.loop_residuals[0] <= 1e-5
    new = loc.trajectory.double().numpy()
    assert new.shape == (4, 4, 4) and np.array_equal(new[0], old[0])
    assert np.abs(new[3] - aligned.double().numpy()).max() <= 2e-5
    assert torch.equal(r.c2w, loc.trajectory[3]) and abs(r.eT - 0.03) <= 1e-4  # 3 cm from the drifted "ground truth"
    # ... and the frames in between have moved towards the truth
    for k in (1, 2):
        assert np.linalg.norm(new[k][:3, 3] - truth[k][:3, 3]) < np.linalg.norm(old[k][:3, 3] - truth[k][:3, 3])
    # the map: frame 0's rows keep every bit, the rows of frames 1 and 2 moved; frame 3's rows carry its index
    c = r.loop_correction
    assert isinstance(c, TrajectoryCorrection) and (c.moved, c.outside, c.frames) == (2 * H, 0, 3)
    assert torch.equal(loc.map.points[:W * H], rows_before[:W * H])
    assert not torch.equal(loc.map.points[W * H:n_before], rows_before[W * H:])
    assert r.added == H and (loc.map.origins[n_before:loc.map.n_live] == 3).all()
    # the insertion render was made at the corrected pose, from the moved rows
    render = loc._render_map.calls[-1]
    assert torch.equal(render["c2w"][0], loc.trajectory[3]) and torch.equal(render["points"], loc.map.points[:n_before])
    # the odometry stays what was tracked
    assert len(loc._odometry) == 3 and np.array_equal(loc._odometry[2], np.linalg.inv(old[2]) @ drift[3].double().numpy())
    # the next frame starts from the corrected pose, and waits
    r4 = loc.track(sequence[4][0], sequence[4][1], gt_c2w=sequence[4][2])
    assert torch.equal(r4.init_c2w, loc.trajectory[3]) and r4.loop_status == "waiting" and r4.loop is False


def test_add_loop(sequence, monkeypatch):  # noqa: F811
    loc = _localizer(MapConfig(origins=True, loop_weight=100.0, loop_by="path"), monkeypatch)
    loc.reset(*sequence[0])
    for k in range(1, base.N_FRAMES):
        loc.track(sequence[k][0], sequence[k][1], gt_c2w=sequence[k][2])
    old = loc.trajectory.double().numpy()
    target = map_correct_ref.twist(1.0, 0.03) @ old[4]
    out = loc.add_loop(1, 4, torch.from_numpy(target))
    assert isinstance(out, TrajectoryCorrection) and out.frames == 3 and out.moved == 3 * H
    assert loc._loops[0][3] == 100.0 and loc._loops[0][:2] == (1, 4)
    new = loc.trajectory.double().numpy()
    assert np.array_equal(new[:2], old[:2]) and np.abs(new[4] - target).max() <= 5e-3  # weight 100: nearly there
    first = loc.last_pose_graph
    # a second edge with an earlier anchor: both are kept, the frames up to the smaller anchor are held
    out = loc.add_loop(0, 3, torch.from_numpy(map_correct_ref.twist(0.5, 0.01) @ new[3]), weight=1e4)
    assert len(loc._loops) == 2 and loc._loops[1][3] == 1e4 and loc.last_pose_graph is not first
    assert loc.last_pose_graph.loop_residuals.shape == (2,)
    assert np.array_equal(loc.trajectory.double().numpy()[0], old[0]) and out.frames == 4
    # what is refused leaves the edges as they were
    for bad in (dict(anchor=3, last=3), dict(anchor=4, last=2), dict(anchor=0, last=9), dict(anchor=-1, last=2),
                dict(anchor=True, last=2), dict(c2w_last=torch.eye(3)), dict(weight=0.0), dict(weight=float("nan")),
                dict(c2w_last=torch.from_numpy(map_correct_ref.twist(120.0, 0.0)) @ loc.trajectory[3].double())):
        a = dict(dict(anchor=0, last=3, c2w_last=loc.trajectory[3], weight=None), **bad)
        with pytest.raises(ValueError):
            loc.add_loop(a["anchor"], a["last"], a["c2w_last"], a["weight"])
    assert len(loc._loops) == 2
    plain = _localizer(MapConfig(), monkeypatch)
    plain.reset(*sequence[0])
    plain.track(sequence[1][0], sequence[1][1], gt_c2w=sequence[1][2])
    with pytest.raises(RuntimeError, match="origins"):
        plain.add_loop(0, 1, torch.eye(4))
    assert plain._odometry == []  # not recorded without the origins


def test_the_option_of_the_evaluation_driver_needs_the_map_mode(tmp_path, capsys):
    from gsplatloc_amd import eval as ev

    with pytest.raises(ValueError, match="map_loop"):
        ev.evaluate_room(None, 200, 3, sequential=True, map_loop=True)
    with pytest.raises(ValueError, match="map_loop_min_gap"):
        ev.evaluate_room(None, 200, 3, sequential=True, map_mode=True, map_loop_min_gap=5)
    for extra in (["--map-loop"], ["--sequential", "--map-loop"], ["--sequential", "--map-loop", "--map-loop-min-gap", "5"]):
        with pytest.raises(SystemExit):
            ev.main(["--root", str(tmp_path)] + extra)
        assert "needs --map" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        ev.main(["--root", str(tmp_path), "--sequential", "--map", "--map-loop-min-gap", "5"])
    assert "needs --map-loop" in capsys.readouterr().err


# ---- the entry point ------------------------------------------------------------------------------------------------
BAD_ARG, OK = -1, 0
GOOD = dict(n_rows=1000, fx=50.0, fy=40.0, cx=31.5, cy=23.5, width=64, height=48, keep=0.95, beyond=1.05,
            near_plane=0.01, n_frames=3)
REFUSED = [("NULL means", dict(means=None)), ("NULL origins", dict(origins=None)), ("NULL w2c", dict(w2c=None)),
           ("NULL depth", dict(depth=None)), ("NULL counts", dict(counts=None)), ("NULL outside", dict(outside=None)),
           ("n_rows < 0", dict(n_rows=-1)), ("n_rows == 2^31", dict(n_rows=1 << 31)), ("n_rows == 2^40", dict(n_rows=1 << 40)),
           ("n_frames == 0", dict(n_frames=0)), ("n_frames < 0", dict(n_frames=-2)),
           ("n_frames > 2^24", dict(n_frames=(1 << 24) + 1)), ("width <= 0", dict(width=0)), ("height <= 0", dict(height=-3)),
           ("2^31 pixels", dict(width=65536, height=32768)), ("fx == 0", dict(fx=0.0)), ("fy == -0", dict(fy=-0.0)),
           ("keep == 0", dict(keep=0.0)), ("keep > 1", dict(keep=1.0000001)), ("NaN keep", dict(keep=float("nan"))),
           ("beyond < 1", dict(beyond=0.9999999)), ("NaN beyond", dict(beyond=float("nan"))),
           ("no rows and no table", dict(n_rows=0, n_frames=0)), ("no rows and NULL means", dict(n_rows=0, means=None))]


def test_the_entry_point_rejects_bad_arguments_before_any_launch(repo_root):
    """Every row is refused on the host: the pointers are one dummy HOST buffer, a launch would give GSL_ERR_HIP or
    worse.  No rows at all is not an error, and launches nothing either."""
    lib = _lib.load_library()
    ret, params = prototypes(repo_root)["gsl_map_covis"]
    assert ret == "int" and [n for _, n in params] == [
        "means", "origins", "n_rows", "w2c", "fx", "fy", "cx", "cy", "depth", "width", "height", "keep", "beyond",
        "near_plane", "n_frames", "counts", "outside", "stream"]
    assert [t.replace(" ", "") for t, _ in params][:4] == ["constfloat*", "constint32_t*", "int64_t", "constfloat*"]
    assert [t.replace(" ", "") for t, _ in params][-4:] == ["int", "int32_t*", "int64_t*", "void*"]
    assert "gsl_map_covis" in _lib.exported_symbols()
    buf = ctypes.create_string_buffer(256)
    for what, over in REFUSED:
        named = dict(GOOD, **over)
        assert set(named) <= {n for _, n in params}, what
        assert lib.gsl_map_covis(*refine_cpu.refine_args(params, named, ctypes.addressof(buf))) == BAD_ARG, what
    assert lib.gsl_map_covis(*refine_cpu.refine_args(params, dict(GOOD, n_rows=0), ctypes.addressof(buf))) == OK
    assert not any(buf.raw)  # nothing wrote to the buffer, the counts included
    assert "map_covis.hip" in open(os.path.join(repo_root, "gsplatloc_amd", "csrc", "Makefile")).read()


# ---- the kernel's budget --------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_the_kernel_stays_in_registers():
    """No scratch, no accumulation registers, eight waves per SIMD; 772 B of LDS (the window's 64 x 3 words and the
    count of rows outside the table) and 19 vector registers are what the build gives ("Covisibility"):
    a change is worth a look."""
    res = _resources("map_covis.hip")
    assert len(res) == 1 and "k_map_covis" in list(res)[0], list(res)
    r = list(res.values())[0]
    assert r["ScratchSize"] == 0 and r["AGPRs"] == 0 and r["Occupancy"] == 8, r
    assert r["VGPRs"] == 19 and r["LDS"] == 772, r
