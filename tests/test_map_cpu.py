"""Frame-to-map localisation, the parts that need no GPU: the mirror of the selection rule on hand-made cases, the
capacity clamp, the argument checks of the two entry points, Localizer(mode="map") around a stand-in tracker, a stand-in
renderer and a map whose device call is the mirror, and the there-and-back sequence."""
import ctypes

import numpy as np
import pytest
import torch

from gsplatloc_amd import _lib
from gsplatloc_amd.data import Parser
from gsplatloc_amd.data.dataset import build_pair
from gsplatloc_amd.data.normalize import align_principle_axes
from gsplatloc_amd.localizer import Localizer
from gsplatloc_amd.mapping import GaussianMap, MapConfig
from gsplatloc_amd.my_gsplat import TrackerConfig
from gsplatloc_amd.my_gsplat.geometry import depth_to_points, init_gs_scales
from gsplatloc_amd.my_gsplat.trainer import TrackResult
from gsplatloc_amd.synthetic import replica_intrinsics, write_replica_sequence, write_replica_there_and_back
from tests import map_ref
from tests.test_abi import prototypes

W, H, N_FRAMES = 32, 24, 5
F32 = np.float32
KEEP = map_ref.keep_of(0.05)


# ---- the mirror of the rule -----------------------------------------------------------------------------------------
def _case(d_o, d_r, a):
    return map_ref.select(np.array(d_o, F32).reshape(2, 3), np.array(d_r, F32).reshape(2, 3),
                          np.array(a, F32).reshape(2, 3), 0.5, KEEP).reshape(-1).tolist()


def test_rule_each_clause_alone():
    # covered everywhere (alpha 0.9), observed depth equal to the map's: nothing is new
    assert _case([2.0] * 6, [2.0] * 6, [0.9] * 6) == [False] * 6
    # first clause alone: alpha below alpha_min on pixels 1 and 4, depths agree
    assert _case([2.0] * 6, [2.0] * 6, [0.9, 0.1, 0.9, 0.9, 0.49999, 0.9]) == [False, True, False, False, True, False]
    # second clause alone: covered, a surface in front of the map's on pixels 0 and 5; BEHIND it (pixel 2) is not new
    assert _case([1.0, 2.0, 3.0, 2.0, 2.0, 1.8], [2.0] * 6, [0.9] * 6) == [True, False, False, False, False, True]


def test_rule_thresholds_are_not_selected():
    """a == alpha_min and d_o == d_r * keep (the float32 product) are not new; one float32 step below each is."""
    limit = F32(2.0) * KEEP
    below = np.nextafter(limit, F32(0))
    assert _case([2.0] * 6, [2.0] * 6, [0.5] * 6) == [False] * 6
    assert _case([2.0] * 6, [2.0] * 6, [np.nextafter(F32(0.5), F32(0))] * 6) == [True] * 6
    assert _case([limit] * 3 + [below] * 3, [2.0] * 6, [0.9] * 6) == [False] * 3 + [True] * 3
    # the product is the float32 one: 1 - 0.05 is not a float32 number, and the double product lies elsewhere
    assert float(limit) != 2.0 * (1.0 - 0.05) and limit.dtype == F32


def test_rule_invalid_depths_are_never_selected():
    bad = [0.0, -1.0, np.nan, np.inf, -np.inf, -0.0]
    assert _case(bad, [2.0] * 6, [0.0] * 6) == [False] * 6  # not covered at all, and still not new
    assert _case(bad, [np.inf] * 6, [0.9] * 6) == [False] * 6
    assert map_ref.select(np.array(bad, F32).reshape(2, 3)).reshape(-1).tolist() == [False] * 6  # no render yet
    # a NaN in the render selects nothing by itself
    assert _case([2.0] * 6, [np.nan] * 6, [np.nan] * 6) == [False] * 6
    # no render yet: every valid pixel
    assert map_ref.select(np.array([1.0, 0.0, 2.0, np.nan, 3.0, -1.0], F32).reshape(2, 3)).reshape(-1).tolist() == [
        True, False, True, False, True, False]


def test_clamp_and_raster_order():
    assert map_ref.clamp(100, 7, 17) == 10 and map_ref.clamp(5, 7, 17) == 5 and map_ref.clamp(5, 17, 17) == 0
    d_o = np.array([[1.0, 0.0, 2.0], [3.0, 4.0, np.nan]], F32)
    rgb = np.arange(18, dtype=F32).reshape(2, 3, 3) * 10
    c2w = np.eye(4, dtype=F32)
    c2w[:3, 3] = [1.0, 2.0, 3.0]
    r = map_ref.insert(d_o, rgb, (2.0, 4.0, 1.0, 0.5), c2w, n_live=1, capacity=4)
    assert r["idx"].tolist() == [0, 2, 3, 4] and r["n_new"] == (4, 3)
    # pixel (u, v) = (0, 0), (2, 0), (0, 1): ((u - 1) / 2 * d, (v - 0.5) / 4 * d, d) + t
    want = [[-0.5 + 1, -0.125 + 2, 1.0 + 3], [1.0 + 1, -0.25 + 2, 2.0 + 3], [-1.5 + 1, 0.375 + 2, 3.0 + 3]]
    assert np.allclose(r["means"], want, atol=1e-12)
    assert np.allclose(r["colors"], rgb.reshape(-1, 3)[[0, 2, 3]] / 255.0, atol=1e-12)
    assert r["means"].shape == r["bound"].shape == (3, 3) and (r["bound"] > 0).all() and (r["bound"] < 1e-5).all()


# ---- the entry points' argument checks ------------------------------------------------------------------------------
BAD_ARG = -1
_SELECT = dict(width=64, height=48, alpha_min=0.5, keep=0.95, ws_bytes="full")
_APPEND = dict(width=64, height=48, fx=50.0, fy=40.0, cx=31.5, cy=23.5, n_live=10, capacity=100, ws_bytes="full")
_ROWS = [
    ("gsl_map_select", "NULL depth", dict(depth=None)), ("gsl_map_select", "NULL n_new", dict(n_new=None)),
    ("gsl_map_select", "NULL ws", dict(ws=None)), ("gsl_map_select", "width <= 0", dict(width=0)),
    ("gsl_map_select", "height <= 0", dict(height=-3)), ("gsl_map_select", "short workspace", dict(ws_bytes=8)),
    ("gsl_map_select", "alphas without render_depth", dict(render_depth=None)),
    ("gsl_map_select", "render_depth without alphas", dict(alphas=None)),
    ("gsl_map_select", "2^31 pixels", dict(width=65536, height=32768)),
    ("gsl_map_append", "NULL depth", dict(depth=None)), ("gsl_map_append", "NULL rgb", dict(rgb=None)),
    ("gsl_map_append", "NULL c2w", dict(c2w=None)), ("gsl_map_append", "NULL means", dict(means=None)),
    ("gsl_map_append", "NULL colors", dict(colors=None)), ("gsl_map_append", "NULL n_new", dict(n_new=None)),
    ("gsl_map_append", "NULL ws", dict(ws=None)), ("gsl_map_append", "width <= 0", dict(width=0)),
    ("gsl_map_append", "height <= 0", dict(height=0)), ("gsl_map_append", "capacity <= 0", dict(capacity=0, n_live=0)),
    ("gsl_map_append", "n_live < 0", dict(n_live=-1)), ("gsl_map_append", "n_live > capacity", dict(n_live=101)),
    ("gsl_map_append", "short workspace", dict(ws_bytes=8)), ("gsl_map_append", "fx == 0", dict(fx=0.0)),
]


def test_workspace_size():
    lib = _lib.load_library()
    # per 256-pixel workgroup: four 64-bit ballots, a count and a base
    assert lib.gsl_map_ws_bytes(640, 480) == 1200 * 40 and lib.gsl_map_ws_bytes(1, 1) == 40
    assert lib.gsl_map_ws_bytes(257, 2) == 3 * 40 and lib.gsl_map_ws_bytes(0, 5) == 40


@pytest.mark.parametrize("fn", ["gsl_map_select", "gsl_map_append"])
def test_entry_points_reject_bad_arguments_before_any_launch(fn, repo_root):
    """Every row is refused on the host (GSL_ERR_BAD_ARG): the pointers are one dummy HOST buffer, a launch would give
    GSL_ERR_HIP or worse."""
    lib = _lib.load_library()
    params = prototypes(repo_root)[fn][1]
    buf = ctypes.create_string_buffer(256)
    rows = [(what, over) for f, what, over in _ROWS if f == fn]
    assert len(rows) >= 9
    for what, over in rows:
        named = dict(_SELECT if fn == "gsl_map_select" else _APPEND, **over)
        assert set(named) <= {n for _, n in params}, (fn, what)
        args = []
        for c_type, name in params:
            if name == "stream":
                args.append(None)
            elif name in named:
                args.append(lib.gsl_map_ws_bytes(named["width"], named["height"]) if named[name] == "full" else named[name])
            else:
                args.append(ctypes.addressof(buf) if "*" in c_type else 0)
        assert getattr(lib, fn)(*args) == BAD_ARG, (fn, what)
    assert not any(buf.raw)  # nothing wrote to the buffer


# ---- Localizer(mode="map") around stand-ins -------------------------------------------------------------------------
class _MirrorMap(GaussianMap):
    """GaussianMap whose device call is the numpy mirror (host tensors)."""
    calls = 0

    def _launch(self, depth, rgb, intr, c2w, render, alphas):
        _MirrorMap.calls += 1
        r = map_ref.insert(depth.numpy(), rgb.numpy(), intr, c2w.numpy(), self.n_live, self.capacity,
                           None if render is None else render.numpy(), None if alphas is None else alphas.numpy(),
                           self.alpha_min, F32(self.keep))
        n = r["n_new"][1]
        self.means[self.n_live:self.n_live + n] = torch.from_numpy(r["means"]).float()
        self.colors[self.n_live:self.n_live + n] = torch.from_numpy(r["colors"]).float()
        return r["n_new"]


class _Tracker:
    """Stands in for GraphTracker: records what it is given; run() answers the reference pose of load_frame -- the ground
    truth of the new frame in the pair's frame -- as the minimum-loss pose."""
    made = []
    best_step = 7

    def __init__(self, N, W_, H_, config, device, render_mode):
        self.args, self.loads = (N, W_, H_, render_mode), []
        _Tracker.made.append(self)

    def load_frame(self, tar_points, colors, scales, src_depth, tar_c2w, src_c2w, K, pixels=None):
        assert tar_points.shape == (self.args[0], 3)
        self.loads.append(dict(tar_points=tar_points.clone(), colors=colors.clone(), scales=scales.clone(),
                               src_depth=src_depth.clone(), tar_c2w=tar_c2w.clone(), src_c2w=src_c2w.clone(),
                               K=K.clone(), pixels=pixels))

    def run(self):
        gt = self.loads[-1]["src_c2w"]
        return TrackResult(best_loss=0.25, steps=12, final_c2w=gt.clone(), best_c2w=gt.clone(),
                           best_step=type(self).best_step)


class _LostTracker(_Tracker):
    best_step = -1


class _Renderer:
    """Stands in for render_depth_alpha: the map covers everything but the first image column, at a depth of 1 cm --
    nothing the camera sees lies in front of that, so only the alpha clause fires: H pixels are new per frame."""

    def __init__(self):
        self.calls = []

    def __call__(self, points, scales, Ks, c2w, height, width):
        self.calls.append(dict(points=points.clone(), scales=scales.clone(), c2w=c2w.clone()))
        alphas = torch.ones(height, width)
        alphas[:, 0] = 0.25
        return torch.full((height, width), 0.01), alphas


@pytest.fixture(scope="module")
def sequence(tmp_path_factory):
    root = tmp_path_factory.mktemp("seq")
    write_replica_sequence(root, W, H, N_FRAMES)
    parser = Parser("Replica", "room0", normalize=False, device="cpu", input_folder=str(root))
    return [parser.frame(i) for i in range(N_FRAMES)]


def _localizer(tracker, renderer, normalize, **kw):
    tracker.made = _Tracker.made = []
    return Localizer(replica_intrinsics(W, H), W, H, TrackerConfig(max_steps=5), normalize=normalize, motion="hold",
                     device="cpu", tracker_factory=tracker, mode="map", map_factory=_MirrorMap, map_renderer=renderer,
                     **kw)


@pytest.mark.parametrize("normalize", [True, False])
def test_map_mode_composition(sequence, normalize, monkeypatch):
    import gsplatloc_amd.data.dataset as DS

    monkeypatch.setattr(DS, "compute_depth_gt", lambda pts, col, Ks, c2w, height, width: torch.zeros(height, width))
    frames, renderer = sequence, _Renderer()
    loc = _localizer(_Tracker, renderer, normalize)
    K = loc.K
    loc.reset(*frames[0])
    # after reset(): every pixel of frame 0 (the room has no invalid depth), placed with its pose, in raster order
    assert loc.map.n_live == W * H and not loc.map.full and loc.map.capacity == 4 * W * H
    want0 = depth_to_points(frames[0][0], K) @ frames[0][2][:3, :3].T + frames[0][2][:3, 3]
    assert torch.allclose(loc.map.points, want0, atol=5e-6)
    assert torch.allclose(loc.map.point_colors, (frames[0][1] / 255.0).reshape(-1, 3), atol=1e-7)
    sizes = [loc.map.n_live]
    for k in range(1, N_FRAMES):
        prefix = loc.map.points.clone()
        r = loc.track(frames[k][0], frames[k][1], gt_c2w=frames[k][2])
        load = _Tracker.made[-1].loads[-1]
        # the target cloud is the live prefix, moved to the pair's frame; the scales are the reference's on that cloud
        T = align_principle_axes(prefix) if normalize else torch.eye(4)
        want = prefix @ T[:3, :3].T + T[:3, 3] if normalize else prefix
        assert load["tar_points"].shape == (sizes[-1], 3) and torch.equal(load["tar_points"], want)
        assert torch.equal(load["scales"], init_gs_scales(want))
        assert torch.equal(load["colors"], loc.map.point_colors[:sizes[-1]])
        # the estimate comes back from the pair's frame: the stand-in answered the ground truth there
        assert not r.lost and r.eT <= 1e-5 and r.eR <= 1e-3
        assert float((loc.trajectory[k] - frames[k][2]).abs().max()) <= 1e-5
        # the map was rendered once, in the pair's frame at the tracker's answer, with the tracker's cloud and scales
        assert len(renderer.calls) == k
        seen = renderer.calls[-1]
        assert torch.equal(seen["points"], load["tar_points"]) and torch.equal(seen["scales"], load["scales"])
        assert torch.equal(seen["c2w"][0], load["src_c2w"])
        # ... and the first column's H pixels were appended, placed with the world estimate
        assert r.added == H and r.map_size == sizes[-1] + H == loc.map.n_live
        col0 = depth_to_points(frames[k][0], K).reshape(H, W, 3)[:, 0]
        assert torch.allclose(loc.map.points[sizes[-1]:], col0 @ r.c2w[:3, :3].T + r.c2w[:3, 3], atol=1e-5)
        assert torch.equal(loc.map.points[:sizes[-1]], prefix)  # live rows are never rewritten
        sizes.append(r.map_size)
    # the live count changed every frame: one tracker per frame, through the factory
    assert [t.args[0] for t in _Tracker.made] == sizes[:-1]
    # reset() starts over
    loc.reset(*frames[1])
    assert loc.map.n_live == W * H and loc.trajectory.shape == (1, 4, 4)


def test_map_mode_a_lost_frame_inserts_nothing(sequence):
    frames, renderer = sequence, _Renderer()
    loc = _localizer(_LostTracker, renderer, False)
    loc.reset(*frames[0])
    before, calls = loc.map.points.clone(), _MirrorMap.calls
    r = loc.track(frames[1][0], frames[1][1])
    assert r.lost and r.added == 0 and r.map_size == W * H == loc.map.n_live
    assert renderer.calls == [] and _MirrorMap.calls == calls and torch.equal(loc.map.points, before)
    assert loc.trajectory.shape == (2, 4, 4)


def test_map_mode_reports_a_full_map(sequence):
    frames = sequence
    loc = _localizer(_Tracker, _Renderer(), False, map_config=MapConfig(capacity=W * H + H + 5))
    loc.reset(*frames[0])
    r1 = loc.track(frames[1][0], frames[1][1], gt_c2w=frames[1][2])
    assert r1.added == H and not loc.map.full
    r2 = loc.track(frames[2][0], frames[2][1], gt_c2w=frames[2][2])
    assert r2.added == 5 and loc.map.full and r2.map_size == loc.map.capacity
    with pytest.raises(ValueError, match="mode"):
        Localizer(replica_intrinsics(W, H), W, H, device="cpu", mode="submap")


def test_a_map_on_the_host_has_no_insert_path(sequence):
    m = GaussianMap(W, H, MapConfig(), "cpu")
    with pytest.raises(AssertionError, match="no CPU path"):
        m.insert_frame(sequence[0][0], sequence[0][1], replica_intrinsics(W, H), torch.eye(4))


def test_frame_mode_calls_the_tracker_as_before(sequence):
    """mode="frame" (and no mode at all): load_frame gets, bit for bit, what build_pair makes of the previous frame placed
    with the previous estimate -- the frame-to-frame arguments -- and the result carries no map figures."""
    frames = sequence
    K = replica_intrinsics(W, H)
    for kw in ({}, {"mode": "frame"}):
        _Tracker.made = []
        loc = Localizer(K, W, H, TrackerConfig(max_steps=5), normalize=False, motion="hold", device="cpu",
                        tracker_factory=_Tracker, **kw)
        assert loc.map is None
        loc.reset(*frames[0])
        for k in range(1, 4):
            placed = loc.trajectory[k - 1].clone()
            r = loc.track(frames[k][0], frames[k][1], gt_c2w=frames[k][2])
            assert r.map_size is None and r.added is None
            (dp, rp, _), (dq, rq, gt) = frames[k - 1], frames[k]
            d = build_pair(depth_to_points(dp, K), (rp / 255.0).reshape(-1, 3), depth_to_points(dq, K),
                           (rq / 255.0).reshape(-1, 3), dq, rq, placed, gt, K, False)
            load = _Tracker.made[0].loads[-1]
            want = dict(tar_points=d.tar_points, colors=d.colors, scales=init_gs_scales(d.tar_points),
                        src_depth=d.src_depth, tar_c2w=placed, src_c2w=gt, K=K)
            for name, v in want.items():
                assert torch.equal(load[name], v), (kw, k, name)
            assert load["pixels"] is None
            assert torch.allclose(d.tar_points, depth_to_points(dp, K) @ placed[:3, :3].T + placed[:3, 3], atol=1e-6)
        assert len(_Tracker.made) == 1 and _Tracker.made[0].args == (W * H, W, H, "ED")


def test_there_and_back_returns_to_the_first_pose(tmp_path):
    poses = write_replica_there_and_back(tmp_path, 16, 12, 3)
    assert poses.shape == (7, 4, 4) and poses.dtype == torch.float64
    assert torch.equal(poses[-1], poses[0]) and torch.equal(poses[0], torch.eye(4, dtype=torch.float64))
    for k in range(3):  # the way back repeats the way out, pose for pose
        assert torch.equal(poses[6 - k], poses[k])
        assert abs(float((poses[k + 1][:3, 3] - poses[k][:3, 3]).norm()) - 0.01) < 1e-4
    parser = Parser("Replica", "room0", normalize=False, device="cpu", input_folder=str(tmp_path))
    assert len(parser) == 6
    first, last = parser.frame(0), parser.frame(6)
    assert torch.equal(first[2], last[2]) and torch.equal(first[0], last[0])  # same pose, same depth image
    assert float((parser.frame(3)[2] - poses[3].float()).abs().max()) <= 1e-6
