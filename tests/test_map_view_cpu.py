"""The local map (tracking against the part of the map that is in view), the parts that need no GPU: the mirror of the
in-view rule on hand-made cases, the workspace size and the argument checks of the two entry points, MapConfig, and
Localizer(mode="map") with ``view_guard_px`` around the stand-in tracker / renderer of tests/test_map_cpu.py and a map
whose device calls are the mirrors.

The composition runs on a there-and-back sequence at 32x24 that turns by 4 degrees per frame (about 1 px at the image
centre, 2 px at its border): on the way out rows leave the guarded view, on the way back -- the stand-in tracker answers
the ground truth, the start pose is the previous one ("hold") -- the view from the estimate reaches rows the start pose
left out unless the guard is wider than that step."""
import ctypes

import numpy as np
import pytest
import torch

from gsplatloc_amd import _lib
from gsplatloc_amd.data import Parser
from gsplatloc_amd.data.normalize import align_principle_axes
from gsplatloc_amd.localizer import Localizer
from gsplatloc_amd.mapping import GaussianMap, MapConfig
from gsplatloc_amd.my_gsplat import TrackerConfig
from gsplatloc_amd.my_gsplat.geometry import init_gs_scales
from gsplatloc_amd.synthetic import replica_intrinsics, write_replica_there_and_back
from tests import map_view_ref as ref
from tests import test_map_cpu as base
from tests.test_abi import prototypes

F32 = np.float32
W, H, N_OUT = 32, 24, 3
NEAR, FAR = TrackerConfig().gs.near_plane, TrackerConfig().gs.far_plane

# ---- the mirror of the rule: power-of-two intrinsics and z = 1, so that u = 64 x + 32 and v = 64 y + 24 are exact ----
RW, RH, INTR, G = 64, 48, (64.0, 64.0, 32.0, 24.0), 8.0
EYE = np.eye(4, dtype=F32)


def _rule(points, guard=G, near=0.5, far=4.0, w2c=EYE):
    return ref.in_view(np.array(points, F32).reshape(-1, 3), w2c, INTR, RW, RH, guard, near, far).tolist()


def _x(u):
    return (u - 32.0) / 64.0


def _y(v):
    return (v - 24.0) / 64.0


def test_rule_each_clause_alone():
    centre = [_x(30.0), _y(20.0), 1.0]
    assert _rule([centre]) == [True]
    # one clause at a time: behind the near plane, beyond the far plane, left, right, above, below
    assert _rule([[0.0, 0.0, 0.25], [0.0, 0.0, 5.0], [_x(-9.0), 0.0, 1.0], [_x(72.0), 0.0, 1.0], [0.0, _y(-9.0), 1.0],
                  [0.0, _y(56.0), 1.0]]) == [False] * 6
    # inside the band but outside the image: in with the guard, out without one
    band = [[_x(-5.0), 0.0, 1.0], [_x(70.0), 0.0, 1.0], [0.0, _y(-7.5), 1.0], [0.0, _y(54.0), 1.0]]
    assert _rule(band) == [True] * 4 and _rule(band, guard=0.0) == [False] * 4
    # behind the camera, where u and v would lie inside the image
    assert _rule([[0.1, 0.1, -1.0]]) == [False]
    # the pose counts: the same point seen from a camera moved 2 m forward lies behind it
    moved = EYE.copy()
    moved[2, 3] = -2.0
    assert _rule([centre], w2c=moved) == [False] and _rule([[0.0, 0.0, 3.0]], w2c=moved) == [True]


def test_rule_borders_are_in_and_the_planes_are_out():
    """u == -guard, u == (width - 1) + guard, v likewise: in (<=); one float32 step of x or y further out: out.
    z == near and z == far: out; one step inside: in."""
    lo_u, hi_u, lo_v, hi_v = _x(-G), _x(RW - 1 + G), _y(-G), _y(RH - 1 + G)
    assert [lo_u, hi_u, lo_v, hi_v] == [-0.625, 0.609375, -0.5, 0.484375]  # exact in float32
    on = [[lo_u, 0.0, 1.0], [hi_u, 0.0, 1.0], [0.0, lo_v, 1.0], [0.0, hi_v, 1.0], [lo_u, lo_v, 1.0], [hi_u, hi_v, 1.0]]
    assert _rule(on) == [True] * 6
    step = lambda a, to: float(np.nextafter(F32(a), F32(to)))  # noqa: E731
    # below: one step of x / y (u = -8 - 2^-18 is a float32); above: the x / y of the first float32 u / v beyond the limit
    # (one step of x there is half a step of u = 71 and rounds back onto the border: the rule is float32's, and in)
    off = [[step(lo_u, -9), 0.0, 1.0], [_x(step(RW - 1 + G, 99)), 0.0, 1.0], [0.0, step(lo_v, -9), 1.0],
           [0.0, _y(step(RH - 1 + G, 99)), 1.0]]
    assert all(float(F32(p[0])) == p[0] and float(F32(p[1])) == p[1] for p in off)  # exact in float32
    assert _rule(off) == [False] * 4
    assert _rule([[step(hi_u, 9), 0.0, 1.0]]) == [True]
    assert _rule([[0.0, 0.0, 0.5], [0.0, 0.0, 4.0]]) == [False, False]
    assert _rule([[0.0, 0.0, step(0.5, 9)], [0.0, 0.0, step(4.0, 0)]]) == [True, True]


def test_rule_nan_and_inf_rows_are_never_selected():
    nan, inf = np.nan, np.inf
    bad = [[nan, 0.0, 1.0], [0.0, nan, 1.0], [0.0, 0.0, nan], [inf, 0.0, 1.0], [0.0, -inf, 1.0], [0.0, 0.0, inf],
           [0.0, 0.0, -inf], [inf, inf, inf], [nan, nan, nan]]
    assert _rule(bad) == [False] * 9 and _rule(bad, far=inf) == [False] * 9
    assert _rule(bad, guard=inf, far=inf) == [False] * 9  # even a band without end
    assert _rule([[0.0, 0.0, 1.0]] + bad)[0] is True


def test_compaction_clamp_and_violation_count():
    pts = np.array([[0.0, 0.0, 1.0], [5.0, 0.0, 1.0], [0.1, 0.1, 1.0], [0.0, 0.0, -1.0], [_x(-3.0), 0.0, 1.0]], F32)
    r = ref.select(pts, EYE, INTR, RW, RH, G, 0.5, 4.0)
    assert r["mask"].tolist() == [True, False, True, False, True] and r["ids"].tolist() == [0, 2, 4]
    assert r["counters"] == (3, 0, 3) and r["ids"].dtype == np.int32
    assert ref.select(pts, EYE, INTR, RW, RH, G, 0.5, 4.0, out_capacity=2)["ids"].tolist() == [0, 2]
    assert ref.select(pts, EYE, INTR, RW, RH, G, 0.5, 4.0, out_capacity=2)["counters"] == (3, 0, 2)
    assert ref.select(pts, EYE, INTR, RW, RH, G, 0.5, 4.0, out_capacity=0)["counters"] == (3, 0, 0)
    # rows in view now that an earlier selection left out: rows 2 and 4 of (0, 2, 4) against (0, 1)
    prev = np.array([True, True, False, False, False])
    assert ref.select(pts, EYE, INTR, RW, RH, G, 0.5, 4.0, prev=prev)["counters"] == (3, 2, 3)
    assert ref.violations(pts, EYE, INTR, RW, RH, G, 0.5, 4.0, r["mask"]) == 0
    assert ref.violations(pts, EYE, INTR, RW, RH, 0.0, 0.5, 4.0, np.zeros(5, bool)) == 2
    c2w = np.eye(4)
    c2w[:3, 3] = [0.5, -1.0, 2.0]
    assert np.array_equal(ref.w2c_of(c2w)[:3, 3], np.array([-0.5, 1.0, -2.0], F32)) and ref.w2c_of(c2w).dtype == F32


def test_the_mirror_carries_the_largest_gpu_cases():
    """66 000 rows, the largest count of tests/test_gpu_map_view.py (258 workgroups: two counts per thread of the scan,
    threads from 129 on idle), on the mirror alone: every pattern is what it says, the count stays below the capacity
    of n + 3 rows the GPU test gives its outputs (so the rows behind it, and the guard rows, keep their sentinels), no
    selected row holds the sentinel value, and the scene of the violation test has what that test asserts."""
    from tests import test_gpu_map_view as gpu

    n = max(gpu.ROWS)
    assert n == 66000 and (n + 255) // 256 == 258
    for pattern in gpu.PATTERNS:
        means, c2w, intr, w, h, intended = gpu._case(n, pattern)
        args = (means, ref.w2c_of(c2w), intr, w, h, gpu.GUARD, gpu.NEAR, gpu.FAR)
        want = ref.select(*args, out_capacity=n + 3)
        if intended is not None:
            assert np.array_equal(want["mask"], intended), pattern
        else:
            assert 0.1 < want["mask"].mean() < 0.8, pattern
        sel, ids = want["counters"][0], want["ids"]
        assert want["counters"] == (sel, 0, sel) and sel <= n < n + 3, pattern
        assert ids.dtype == np.int32 and len(ids) == sel and (np.diff(ids) > 0).all() and (sel == 0 or ids[-1] < n)
        assert not (means[ids] == gpu.SENTINEL).any() and not (ids == -77).any(), pattern
        assert ref.select(*args, out_capacity=sel // 2)["counters"] == (sel, 0, sel // 2), pattern
    means, colors, w2c_a, w2c_b = gpu._violation_case(n)
    assert means.shape == colors.shape == (n, 3) and not (colors == gpu.SENTINEL).any()
    geom = (gpu.INTR, gpu.W, gpu.H)
    mask_a = ref.in_view(means, w2c_a, *geom, gpu.GUARD, gpu.NEAR, gpu.FAR)
    assert 0.2 < mask_a.mean() < 0.8
    b = ref.select(means, w2c_b, *geom, 4.0, gpu.NEAR, gpu.FAR, prev=mask_a)["counters"]
    assert 0 < b[1] < b[0] < n
    same = ref.select(means, w2c_a, *geom, 4.0, gpu.NEAR, gpu.FAR, prev=mask_a)["counters"]
    assert same[1] == 0 and 0 < same[0] <= int(mask_a.sum())
    wider = ref.select(means, w2c_a, *geom, 20.0, gpu.NEAR, gpu.FAR, prev=mask_a)["counters"]
    assert wider[1] == wider[0] - int(mask_a.sum()) > 0


# ---- the entry points' argument checks ------------------------------------------------------------------------------
BAD_ARG, WORKSPACE = -1, -2
_SELECT = dict(n_rows=1000, fx=50.0, fy=40.0, cx=31.5, cy=23.5, width=64, height=48, guard_px=8.0, near_plane=0.01,
               far_plane=100.0, prev_ws=None, ws_bytes="full")
_GATHER = dict(n_rows=1000, out_capacity=1000, ws_bytes="full")
S, GA = "gsl_map_view_select", "gsl_map_view_gather"
_ROWS = [
    (S, "NULL means", dict(means=None), BAD_ARG), (S, "NULL w2c", dict(w2c=None), BAD_ARG),
    (S, "NULL counters", dict(counters=None), BAD_ARG), (S, "NULL ws", dict(ws=None), BAD_ARG),
    (S, "n_rows == 0", dict(n_rows=0), BAD_ARG), (S, "n_rows < 0", dict(n_rows=-5), BAD_ARG),
    (S, "n_rows == 2^31", dict(n_rows=1 << 31), BAD_ARG), (S, "n_rows beyond 2^32", dict(n_rows=(1 << 32) + 7), BAD_ARG),
    (S, "width <= 0", dict(width=0), BAD_ARG), (S, "height <= 0", dict(height=-3), BAD_ARG),
    (S, "fx == 0", dict(fx=0.0), BAD_ARG), (S, "fy == 0", dict(fy=0.0), BAD_ARG),
    (S, "negative guard", dict(guard_px=-0.5), BAD_ARG), (S, "NaN guard", dict(guard_px=float("nan")), BAD_ARG),
    (S, "near == far", dict(near_plane=2.0, far_plane=2.0), BAD_ARG),
    (S, "near > far", dict(near_plane=3.0, far_plane=2.0), BAD_ARG),
    (S, "NaN near", dict(near_plane=float("nan")), BAD_ARG), (S, "prev_ws == ws", dict(prev_ws="buffer"), BAD_ARG),
    (S, "short workspace", dict(ws_bytes=8), WORKSPACE),
    (S, "workspace one byte short", dict(ws_bytes="short"), WORKSPACE),
    (GA, "NULL means", dict(means=None), BAD_ARG), (GA, "NULL colors", dict(colors=None), BAD_ARG),
    (GA, "NULL out_means", dict(out_means=None), BAD_ARG), (GA, "NULL out_colors", dict(out_colors=None), BAD_ARG),
    (GA, "NULL counters", dict(counters=None), BAD_ARG), (GA, "NULL ws", dict(ws=None), BAD_ARG),
    (GA, "n_rows == 0", dict(n_rows=0), BAD_ARG), (GA, "n_rows == 2^31", dict(n_rows=1 << 31), BAD_ARG),
    (GA, "out_capacity < 0", dict(out_capacity=-1), BAD_ARG), (GA, "short workspace", dict(ws_bytes=8), WORKSPACE),
    (GA, "workspace one byte short", dict(ws_bytes="short"), WORKSPACE),
]


def test_workspace_size():
    lib = _lib.load_library()
    # per 256-row workgroup: four 64-bit ballots, two counts and their two bases
    assert lib.gsl_map_view_ws_bytes(1) == 48 and lib.gsl_map_view_ws_bytes(256) == 48
    assert lib.gsl_map_view_ws_bytes(257) == 96 and lib.gsl_map_view_ws_bytes(1_000_000) == 3907 * 48
    assert lib.gsl_map_view_ws_bytes((1 << 31) - 1) == (1 << 23) * 48
    assert lib.gsl_map_view_ws_bytes(0) == 48 and lib.gsl_map_view_ws_bytes(-4) == 48
    assert lib.gsl_map_view_ws_bytes(1 << 31) == 48  # not a row count the entry points take


@pytest.mark.parametrize("fn", [S, GA])
def test_entry_points_reject_bad_arguments_before_any_launch(fn, repo_root):
    """Every row is refused on the host: the pointers are one dummy HOST buffer, a launch would give GSL_ERR_HIP or
    worse."""
    lib = _lib.load_library()
    params = prototypes(repo_root)[fn][1]
    buf = ctypes.create_string_buffer(256)
    rows = [(what, over, want) for f, what, over, want in _ROWS if f == fn]
    assert len(rows) >= 11
    for what, over, want in rows:
        named = dict(_SELECT if fn == S else _GATHER, **over)
        assert set(named) <= {n for _, n in params}, (fn, what)
        full = lib.gsl_map_view_ws_bytes(named["n_rows"])
        args = []
        for c_type, name in params:
            if name == "stream":
                args.append(None)
            elif name in named:
                args.append({"full": full, "short": full - 1, "buffer": ctypes.addressof(buf)}.get(named[name], named[name])
                            if isinstance(named[name], str) else named[name])
            else:
                args.append(ctypes.addressof(buf) if "*" in c_type else 0)
        assert getattr(lib, fn)(*args) == want, (fn, what)
    assert not any(buf.raw)  # nothing wrote to the buffer


def test_map_config_validation():
    assert MapConfig().view_guard_px is None and MapConfig().view_reach_px == 4.0
    assert MapConfig(view_guard_px=4.0).view_guard_px == 4.0  # the smallest legal guard is the reach
    assert MapConfig(view_guard_px=1.0, view_reach_px=0.5).view_reach_px == 0.5
    for kw in (dict(view_guard_px=3.9), dict(view_guard_px=0.0), dict(view_guard_px=8.0, view_reach_px=8.5),
               dict(view_guard_px=-1.0, view_reach_px=-2.0), dict(view_guard_px=float("nan")),
               dict(view_reach_px=float("nan")), dict(view_reach_px=-1.0)):
        with pytest.raises(ValueError, match="view_"):
            MapConfig(**kw)
    m = GaussianMap(W, H, MapConfig(), "cpu")
    m.n_live = 3
    with pytest.raises(AssertionError, match="no CPU path"):
        m.select_view(replica_intrinsics(W, H), torch.eye(4), 8.0, NEAR, FAR)
    with pytest.raises(RuntimeError, match="select_view"):
        GaussianMap(W, H, MapConfig(), "cpu").view_violations(replica_intrinsics(W, H), torch.eye(4), NEAR, FAR)


# ---- Localizer(mode="map", view_guard_px) around stand-ins ----------------------------------------------------------
class _ViewMirrorMap(base._MirrorMap):
    """GaussianMap whose device calls are the numpy mirrors; records the view calls and what insert_frame rendered."""
    view_calls, renders = [], []

    def _launch(self, depth, rgb, intr, c2w, render, alphas):
        _ViewMirrorMap.renders.append(None if render is None else render.clone())
        return super()._launch(depth, rgb, intr, c2w, render, alphas)

    def _view_launch(self, intr, w2c, guard_px, near, far, check):
        v = self._view_buffers()
        r = ref.select(self.means[:self.n_live].numpy(), w2c.numpy(), intr, self.W, self.H, guard_px, near, far,
                       out_capacity=self.capacity, prev=self._mask if check else None)
        _ViewMirrorMap.view_calls.append(dict(check=check, w2c=w2c.numpy().copy(), guard=guard_px, near=near, far=far,
                                              counters=r["counters"]))
        if not check:
            self._mask, ids = r["mask"], torch.from_numpy(r["ids"]).long()
            v["means"][:len(ids)], v["colors"][:len(ids)] = self.means[ids], self.colors[ids]
            v["ids"][:len(ids)] = torch.from_numpy(r["ids"])
        return r["counters"]


class _CountingRenderer(base._Renderer):
    """The stand-in renderer of tests/test_map_cpu.py whose depth image names the call it came from."""

    def __call__(self, points, scales, Ks, c2w, height, width):
        depth, alphas = super().__call__(points, scales, Ks, c2w, height, width)
        return depth * len(self.calls), alphas


@pytest.fixture(scope="module")
def sequence(tmp_path_factory):
    root = tmp_path_factory.mktemp("view_seq")
    write_replica_there_and_back(root, W, H, N_OUT, rot_deg=4.0, trans=0.01)
    parser = Parser("Replica", "room0", normalize=False, device="cpu", input_folder=str(root))
    return [parser.frame(i) for i in range(2 * N_OUT + 1)]


def _localizer(tracker, renderer, normalize, map_config, map_factory=_ViewMirrorMap):
    tracker.made = base._Tracker.made = []
    _ViewMirrorMap.view_calls, _ViewMirrorMap.renders = [], []
    return Localizer(replica_intrinsics(W, H), W, H, TrackerConfig(max_steps=5), normalize=normalize, motion="hold",
                     device="cpu", tracker_factory=tracker, mode="map", map_factory=map_factory, map_renderer=renderer,
                     map_config=map_config)


def _intr():
    K = replica_intrinsics(W, H)
    return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])


def _mask(points, c2w, guard):
    return ref.in_view(points.numpy(), ref.w2c_of(c2w.numpy()), _intr(), W, H, guard, NEAR, FAR)


def _moved(points, normalize):
    if not normalize:
        return points
    T = align_principle_axes(points)
    return points @ T[:3, :3].T + T[:3, 3]


def _drive(frames, normalize, config, monkeypatch):
    """Tracks the sequence and checks, frame by frame, what the tracker, the renderer and insert_frame were given
    against the mirror; returns the per-frame results and (tracked, live rows before the frame)."""
    import gsplatloc_amd.data.dataset as DS

    monkeypatch.setattr(DS, "compute_depth_gt", lambda pts, col, Ks, c2w, height, width: torch.zeros(height, width))
    renderer = _CountingRenderer()
    loc = _localizer(base._Tracker, renderer, normalize, config)
    guard, reach = config.view_guard_px, config.view_reach_px
    loc.reset(*frames[0])
    results, sizes = [], []
    for k in range(1, len(frames)):
        prefix, start, n_calls = loc.map.points.clone(), loc.trajectory[k - 1].clone(), len(renderer.calls)
        _ViewMirrorMap.view_calls = []
        r = loc.track(frames[k][0], frames[k][1], gt_c2w=frames[k][2])
        load = base._Tracker.made[-1].loads[-1]
        # the tracker received exactly the mirror's selection at the start pose (motion "hold": the previous estimate)
        tracked = _mask(prefix, start, guard)
        want = _moved(prefix[torch.from_numpy(tracked)], normalize)
        assert r.tracked == int(tracked.sum()) == load["tar_points"].shape[0] == base._Tracker.made[-1].args[0]
        assert torch.equal(load["tar_points"], want) and torch.equal(load["scales"], init_gs_scales(want))
        assert torch.equal(load["colors"], loc.map.point_colors[:len(prefix)][torch.from_numpy(tracked)])
        assert not r.lost and r.eT <= 1e-5 and float((r.init_c2w - start).abs().max()) == 0.0
        # the check: the reach at the estimate against the tracked rows
        at_est = _mask(prefix, r.c2w, reach)
        assert r.view_violations == int((at_est & ~tracked).sum())
        calls = _ViewMirrorMap.view_calls
        assert [c["check"] for c in calls] == [False, True] + ([False] if r.view_violations else [])
        assert [c["guard"] for c in calls] == [guard, reach] + ([guard] if r.view_violations else [])
        assert all(c["near"] == NEAR and c["far"] == FAR for c in calls)
        assert np.array_equal(calls[0]["w2c"], ref.w2c_of(start.numpy()))
        assert all(np.array_equal(c["w2c"], ref.w2c_of(r.c2w.numpy())) for c in calls[1:])
        # one render per frame: of the tracked set, or of the selection made at the estimate
        assert len(renderer.calls) == n_calls + 1
        seen = renderer.calls[-1]
        if r.view_violations == 0:
            assert torch.equal(seen["points"], load["tar_points"]) and torch.equal(seen["scales"], load["scales"])
            assert torch.equal(seen["c2w"][0], load["src_c2w"])
        else:
            again = _mask(prefix, r.c2w, guard)
            assert not np.array_equal(again, tracked) and not (at_est & ~again).any()  # it covers the view now
            want = _moved(prefix[torch.from_numpy(again)], normalize)
            assert torch.equal(seen["points"], want) and torch.equal(seen["scales"], init_gs_scales(want))
            if not normalize:
                assert torch.equal(seen["c2w"][0], r.c2w)
        # insert_frame got that render (the stand-in's depth image names its call; pca_factor is 1 without normalize)
        if not normalize:
            assert torch.equal(_ViewMirrorMap.renders[-1], torch.full((H, W), 0.01) * len(renderer.calls))
        assert r.added == H and r.map_size == len(prefix) + H == loc.map.n_live
        assert torch.equal(loc.map.points[:len(prefix)], prefix)  # live rows are never rewritten
        results.append(r)
        sizes.append((r.tracked, len(prefix)))
    return results, sizes


@pytest.mark.parametrize("normalize", [False, True])
def test_view_mode_tracks_the_selection_and_renders_it(sequence, normalize, monkeypatch):
    """A guard wider than the step plus the reach: no violation anywhere, one render per frame of the tracked set --
    and from the third frame on the tracker sees fewer rows than the map has."""
    results, sizes = _drive(sequence, normalize, MapConfig(view_guard_px=4.0, view_reach_px=0.5), monkeypatch)
    assert [r.view_violations for r in results] == [0] * (2 * N_OUT)
    assert sizes[0][0] == sizes[0][1] == W * H  # frame 0 seen from its own pose: everything
    assert all(t <= n for t, n in sizes) and sum(t < n for t, n in sizes) >= 3, sizes


@pytest.mark.parametrize("normalize", [False, True])
def test_view_mode_renders_a_selection_at_the_estimate_when_the_band_fails(sequence, normalize, monkeypatch):
    """The smallest legal guard (the reach) and the same steps: on the way back the view from the estimate reaches rows
    the start pose left out; the render that goes into insert_frame is made from a selection at the estimate."""
    results, sizes = _drive(sequence, normalize, MapConfig(view_guard_px=4.0, view_reach_px=4.0), monkeypatch)
    v = [r.view_violations for r in results]
    assert sum(x > 0 for x in v[N_OUT:]) >= 2, v
    assert all(t <= n for t, n in sizes) and any(t < n for t, n in sizes), sizes


def test_view_mode_a_lost_frame_checks_and_renders_nothing(sequence):
    frames, renderer = sequence, base._Renderer()
    loc = _localizer(base._LostTracker, renderer, False, MapConfig(view_guard_px=8.0))
    loc.reset(*frames[0])
    before, inserts = loc.map.points.clone(), base._MirrorMap.calls
    r = loc.track(frames[1][0], frames[1][1])
    assert r.lost and r.added == 0 and r.map_size == W * H == loc.map.n_live
    assert r.tracked == W * H and r.view_violations is None
    assert [c["check"] for c in _ViewMirrorMap.view_calls] == [False]  # the selection before tracking, nothing after
    assert renderer.calls == [] and base._MirrorMap.calls == inserts and torch.equal(loc.map.points, before)


def test_view_mode_an_empty_selection_falls_back_to_the_whole_map(sequence):
    """A map that lies behind the start pose altogether: the tracker gets every live row."""
    frames = sequence
    loc = _localizer(base._Tracker, base._Renderer(), False, MapConfig(view_guard_px=4.0))
    loc.reset(*frames[0])
    loc.map.means[:loc.map.n_live] *= torch.tensor([-1.0, 1.0, -1.0])  # half a turn about y: behind the camera now
    r = loc.track(frames[1][0], frames[1][1])
    assert _ViewMirrorMap.view_calls[0]["counters"][0] == 0 and r.tracked == W * H and r.view_violations == 0
    assert base._Tracker.made[-1].loads[-1]["tar_points"].shape == (W * H, 3)


def test_without_the_option_the_calls_are_those_of_the_map_mode(sequence, monkeypatch):
    """view_guard_px=None: tracker loads, renders and inserted rows are, bit for bit, those of a map without the view
    entry points at all (tests/test_map_cpu.py's mirror map); nothing is selected or checked."""
    import gsplatloc_amd.data.dataset as DS

    monkeypatch.setattr(DS, "compute_depth_gt", lambda pts, col, Ks, c2w, height, width: torch.zeros(height, width))
    runs = []
    for factory in (base._MirrorMap, _ViewMirrorMap):
        renderer = base._Renderer()
        loc = _localizer(base._Tracker, renderer, True, MapConfig(), map_factory=factory)
        loc.reset(*sequence[0])
        results = [loc.track(f[0], f[1], gt_c2w=f[2]) for f in sequence[1:4]]
        assert _ViewMirrorMap.view_calls == []
        assert all(r.view_violations is None for r in results)
        assert [r.tracked for r in results] == [W * H + k * H for k in range(3)]
        loads = [t.loads[-1] for t in base._Tracker.made]
        runs.append((loads, renderer.calls, loc.map.points.clone(), loc.trajectory.clone()))
    (loads_a, renders_a, points_a, traj_a), (loads_b, renders_b, points_b, traj_b) = runs
    assert len(loads_a) == len(loads_b) == 3 and len(renders_a) == len(renders_b) == 3
    for a, b in zip(loads_a + renders_a, loads_b + renders_b):
        assert a.keys() == b.keys()
        for name in a:
            assert (a[name] is None and b[name] is None) or torch.equal(a[name], b[name]), name
    assert torch.equal(points_a, points_b) and torch.equal(traj_a, traj_b)
