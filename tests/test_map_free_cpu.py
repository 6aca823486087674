"""Free space (the rows of the map a frame sees through are removed), the parts that need no GPU: the mirror of the rule
on hand-made cases, the argument checks of the entry point, MapConfig, GaussianMap.remove_seen_through and
Localizer(mode="map") with ``free_rho`` around the stand-in tracker / renderer of tests/test_map_cpu.py and a map whose
device calls are the mirrors, and the register budget of the kernel.

The hand-made cases: a 6x4 image, the identity pose, intrinsics (4, 4, 2, 1) -- u = 4 x / z + 2, v = 4 y / z + 1 -- and
dyadic rows, so that every product, quotient and sum of the rule is exact and a row sits where the case says."""
import ctypes

import numpy as np
import pytest
import torch

from gsplatloc_amd import _lib
from gsplatloc_amd.localizer import Localizer
from gsplatloc_amd.mapping import GaussianMap, MapConfig
from gsplatloc_amd.my_gsplat import TrackerConfig
from gsplatloc_amd.synthetic import panel_depth, replica_intrinsics, room_depth, write_replica_vanishing_panel
from tests import map_free_ref as ref
from tests import test_map_cpu as base
from tests.test_abi import prototypes
from tests.test_kernel_resources import HIPCC, _resources
from tests.test_map_cpu import sequence  # noqa: F401  (the 32x24 drifting sequence, a module fixture there)

F32 = np.float32
RW, RH, INTR = 6, 4, (4.0, 4.0, 2.0, 1.0)
EYE = np.eye(4, dtype=F32)
KEEP = ref.keep_of(0.05)
NEAR = 0.25
FREE = np.full((RH, RW), 2.0, F32)  # a surface at 2 m everywhere: a row at z = 1 is seen through


def _p(u, v, z=1.0):
    """The row that projects onto (u, v) at depth z (exact for dyadic u, v, z)."""
    return [(u - 2.0) / 4.0 * z, (v - 1.0) / 4.0 * z, z]


def _kept(points, depth=FREE, window=1, keep=KEEP, near=NEAR, w2c=EYE):
    return ref.rule(np.array(points, F32).reshape(-1, 3), w2c, INTR, depth, keep, window, near)[0].tolist()


def _tested(points, depth=FREE, window=1, near=NEAR):
    return ref.rule(np.array(points, F32).reshape(-1, 3), EYE, INTR, depth, KEEP, window, near)[1].tolist()


def _with(depth, **pixels):
    d = np.array(depth, F32).copy()
    for at, value in pixels.items():
        u, v = int(at[1]), int(at[2])  # "p32" = column 3, line 2
        d[v, u] = value
    return d


# ---- the mirror of the rule -----------------------------------------------------------------------------------------
def test_rule_each_clause_alone():
    centre = _p(3, 2)
    # tested, nothing in the way: removed
    assert _kept([centre]) == [False] and _tested([centre]) == [True]
    # on the observed surface, and behind it: blocked by its own pixel
    assert _kept([_p(3, 2, 2.0), _p(3, 2, 4.0)]) == [True, True] and _tested([_p(3, 2, 2.0)]) == [True]
    # untested: behind the camera, outside the image on each of the four sides
    out = [[0.25, 0.25, -1.0], _p(-1, 2), _p(6, 2), _p(3, -1), _p(3, 4)]
    assert _kept(out) == [True] * 5 and _tested(out) == [False] * 5
    # one pixel of the window closer than the row: blocked
    assert _kept([centre], _with(FREE, p21=0.5)) == [True]
    assert _kept([centre], _with(FREE, p21=0.5), window=0) == [False]  # ... and outside a window of one pixel
    # the pose counts: seen from a camera 1.5 m further back the same row lies behind the surface at 2 m
    moved = EYE.copy()
    moved[2, 3] = 1.5
    assert _kept([[0.0, 0.0, 1.0]], w2c=moved) == [True] and _kept([[0.0, 0.0, 0.25]], w2c=moved) == [False]


def test_rule_threshold_is_kept():
    """z == d * keep (the float32 product) stays; one float32 step below goes."""
    limit = F32(2.0) * KEEP
    below = np.nextafter(limit, F32(0))
    assert limit.dtype == F32 and float(limit) != 2.0 * (1.0 - 0.05)  # the product is float32's
    for window in (0, 1):
        assert _kept([_p(2, 1, float(limit)), _p(2, 1, float(below))], window=window) == [True, False]
    # keep == 1 (free_rho -> 0): a row on the surface stays, one step in front goes
    one = F32(1.0)
    assert _kept([_p(2, 1, 2.0), _p(2, 1, float(np.nextafter(F32(2.0), F32(0))))], keep=one) == [True, False]


def test_rule_rounds_half_to_even():
    """u = 2.5 is column 2 and u = 3.5 is column 4 (rint); window 0, so only the row's own pixel can block."""
    col = lambda c: _with(FREE, **{f"p{c}1": 0.5})  # noqa: E731  the pixel (c, 1) blocks
    half2, half3 = _p(2.5, 1), _p(3.5, 1)
    assert _kept([half2], col(2), 0) == [True] and _kept([half2], col(3), 0) == [False]
    assert _kept([half3], col(4), 0) == [True] and _kept([half3], col(3), 0) == [False]
    # lines likewise: v = 0.5 is line 0, v = 1.5 is line 2
    assert _kept([_p(2, 0.5)], _with(FREE, p20=0.5), 0) == [True] and _kept([_p(2, 0.5)], _with(FREE, p21=0.5), 0) == [False]
    assert _kept([_p(2, 1.5)], _with(FREE, p22=0.5), 0) == [True] and _kept([_p(2, 1.5)], _with(FREE, p21=0.5), 0) == [False]


def test_rule_minus_zero_is_column_zero():
    """u = -0.5 rounds to -0, passes >= 0 and is tested at column 0; the next float32 u below rounds to -1."""
    on = _p(-0.5, 1)
    off = [float(np.nextafter(F32(on[0]), F32(-9))), on[1], 1.0]
    u_off = F32(4.0) * F32(off[0]) / F32(1.0) + F32(2.0)
    assert F32(4.0) * F32(on[0]) + F32(2.0) == F32(-0.5) and u_off == F32(-0.5) - F32(2.0 ** -22)  # -0.50000024
    assert _tested([on, off]) == [True, False]
    assert _kept([on, off], window=0) == [False, True]
    assert _kept([on], _with(FREE, p01=0.5), 0) == [True] and _kept([on], _with(FREE, p11=0.5), 0) == [False]
    # lines: v = -0.5 is line 0; and the far borders: u = W - 1 + 0.5 rounds to W (even), untested
    assert _tested([_p(2, -0.5), _p(5.5, 1), _p(2, 3.5)]) == [True, False, False]
    assert _tested([_p(4.5, 1), _p(2, 2.5)]) == [True, True]  # 4.5 -> 4, 2.5 -> 2


def test_rule_window_is_clipped_at_the_borders():
    """Pixels of the window outside the image are skipped: they neither block nor are they read."""
    edge = [_p(0, 1), _p(RW - 1, 1), _p(2, 0), _p(2, RH - 1), _p(0, 0), _p(RW - 1, RH - 1)]
    for window in (0, 1, 2, 3):
        assert _kept(edge, window=window) == [False] * 6, window
    # what is left of the window still blocks
    assert _kept([_p(0, 1)], _with(FREE, p12=0.5)) == [True] and _kept([_p(RW - 1, 1)], _with(FREE, p40=0.5)) == [True]
    assert _kept([_p(0, 0)], _with(FREE, p11=0.5)) == [True] and _kept([_p(RW - 1, RH - 1)], _with(FREE, p42=0.5)) == [True]


@pytest.mark.parametrize("bad", [0.0, -0.0, -1.0, np.nan, np.inf, -np.inf])
def test_rule_a_pixel_without_depth_blocks(bad):
    """No evidence, no removal: in the centre pixel and in a corner of the window."""
    row = [_p(3, 2)]
    assert _kept(row, _with(FREE, p32=bad)) == [True] and _kept(row, _with(FREE, p32=bad), window=0) == [True]
    assert _kept(row, _with(FREE, p21=bad)) == [True] and _kept(row, _with(FREE, p43=bad)) == [True]
    assert _kept(row, _with(FREE, p21=bad), window=0) == [False]  # outside the window: not looked at
    assert _kept(row, _with(FREE, p00=bad)) == [False]


def test_rule_window_sizes():
    """Only a corner pixel blocks: (1, 1) is the corner of the window of 1 around (2, 2), (0, 0) that of 2."""
    row = [_p(2, 2)]
    assert [_kept(row, _with(FREE, p11=0.5), w) for w in (0, 1, 2, 3)] == [[False], [True], [True], [True]]
    assert [_kept(row, _with(FREE, p00=0.5), w) for w in (0, 1, 2, 3)] == [[False], [False], [True], [True]]
    assert [_kept(row, _with(FREE, p50=0.5), w) for w in (0, 1, 2, 3)] == [[False], [False], [False], [True]]


def test_rule_near_plane_and_non_finite_rows_are_kept():
    assert _kept([[0.0, 0.0, NEAR], [0.0, 0.0, float(np.nextafter(F32(NEAR), F32(9)))]]) == [True, False]
    assert _kept([[0.0, 0.0, 0.0], [0.0, 0.0, -0.5]]) == [True, True]
    nan, inf = np.nan, np.inf
    bad = [[nan, 0.0, 1.0], [0.0, nan, 1.0], [0.0, 0.0, nan], [inf, 0.0, 1.0], [0.0, -inf, 1.0], [0.0, 0.0, inf],
           [0.0, 0.0, -inf], [inf, inf, inf], [nan, nan, nan]]
    assert _kept(bad) == [True] * 9 and _tested(bad) == [False] * 9
    assert _kept(bad, np.full((RH, RW), inf, F32)) == [True] * 9
    assert _kept([[0.0, 0.0, 1.0]] + bad)[0] is False


def test_select_is_the_ascending_list_of_the_rows_that_stay():
    pts = np.array([_p(3, 2), _p(3, 2, 2.0), _p(2, 1), _p(-1, 2), _p(4, 1)], F32)
    r = ref.select(pts, EYE, INTR, FREE, KEEP, 1, NEAR)
    assert r["kept"].tolist() == [False, True, False, True, False] and r["tested"].tolist() == [True, True, True, False, True]
    assert r["ids"].tolist() == [1, 3] and r["ids"].dtype == np.int32 and r["counters"] == (2, 0, 2)
    assert ref.keep_of(0.05).dtype == F32 and ref.keep_of(0.05) == F32(1.0) - F32(0.05)


def test_the_mirror_carries_the_gpu_cases():
    """The cases of tests/test_gpu_map_free.py on the mirror alone: every pattern is what it says, under every window;
    the random cloud at 4099 rows loses between 10 % and 80 % of its tested rows; the hand-made rows get the intended
    verdict; no row that stays holds the sentinel value."""
    from tests import test_gpu_map_free as gpu

    for n in (gpu.ROWS[0], 257, gpu.ROWS[-1]):
        for pattern in gpu.PATTERNS:
            means, c2w, intr, depth, keep, intended = gpu._case(n, pattern)
            for window in gpu.WINDOWS:
                want = ref.select(means, ref.w2c_of(c2w), intr, depth, keep, window, gpu.NEAR)
                if intended is not None:
                    assert np.array_equal(want["kept"], intended) and want["tested"].all(), (n, pattern, window)
                elif n == 4099:
                    gone = (~want["kept"]).sum() / want["tested"].sum()
                    assert 0.1 <= gone <= 0.8 and 0.3 < want["tested"].mean() < 0.95, (window, gone)
                ids = want["ids"]
                assert want["counters"] == (len(ids), 0, len(ids)) and (np.diff(ids) > 0).all()
                assert not (means[ids] == gpu.SENTINEL).any()
    means, where = gpu._random_case(4099)
    rows, stays = gpu._specials()
    assert len(where) == len(rows) == len(stays) == 13
    for window in gpu.WINDOWS:
        kept, tested = ref.rule(means, ref.w2c_of(gpu._exact_pose()), gpu.EINTR, gpu._exact_depth(), gpu.EKEEP, window,
                                gpu.NEAR)
        want = stays.copy()
        if window >= 1:
            want[[4, 5]] = True
        assert kept[where].tolist() == want.tolist(), window
        assert tested[where].tolist() == [True, True, True, False, True, True, True] + [False] * 6
    assert float(F32(gpu.D_STEP) * gpu.EKEEP) == 1.875 + 2.0 ** -22 and float(F32(2.0) * gpu.EKEEP) == 1.875


# ---- the entry point's argument checks ------------------------------------------------------------------------------
BAD_ARG, WORKSPACE = -1, -2
FN = "gsl_map_free_select"
_GOOD = dict(n_rows=1000, fx=50.0, fy=40.0, cx=31.5, cy=23.5, width=64, height=48, keep=0.95, window_px=1,
             near_plane=0.01, ws_bytes="full")
_ROWS = [
    ("NULL means", dict(means=None), BAD_ARG), ("NULL w2c", dict(w2c=None), BAD_ARG),
    ("NULL depth", dict(depth=None), BAD_ARG), ("NULL counters", dict(counters=None), BAD_ARG),
    ("NULL ws", dict(ws=None), BAD_ARG), ("n_rows == 0", dict(n_rows=0), BAD_ARG),
    ("n_rows < 0", dict(n_rows=-5), BAD_ARG), ("n_rows == 2^31", dict(n_rows=1 << 31), BAD_ARG),
    ("n_rows beyond 2^32", dict(n_rows=(1 << 32) + 7), BAD_ARG), ("width <= 0", dict(width=0), BAD_ARG),
    ("height <= 0", dict(height=-3), BAD_ARG), ("2^31 pixels", dict(width=65536, height=32768), BAD_ARG),
    ("fx == 0", dict(fx=0.0), BAD_ARG), ("fy == 0", dict(fy=0.0), BAD_ARG), ("fx == -0", dict(fx=-0.0), BAD_ARG),
    ("keep == 0", dict(keep=0.0), BAD_ARG), ("keep < 0", dict(keep=-0.5), BAD_ARG),
    ("keep > 1", dict(keep=1.0000001), BAD_ARG), ("NaN keep", dict(keep=float("nan")), BAD_ARG),
    ("window < 0", dict(window_px=-1), BAD_ARG), ("window > 3", dict(window_px=4), BAD_ARG),
    ("short workspace", dict(ws_bytes=8), WORKSPACE), ("workspace one byte short", dict(ws_bytes="short"), WORKSPACE),
]


def test_entry_point_rejects_bad_arguments_before_any_launch(repo_root):
    """Every row is refused on the host: the pointers are one dummy HOST buffer, a launch would give GSL_ERR_HIP or
    worse."""
    lib = _lib.load_library()
    params = prototypes(repo_root)[FN][1]
    assert [n for _, n in params] == ["means", "n_rows", "w2c", "fx", "fy", "cx", "cy", "depth", "width", "height", "keep",
                                      "window_px", "near_plane", "counters", "ws", "ws_bytes", "stream"]
    buf = ctypes.create_string_buffer(256)
    for what, over, want in _ROWS:
        named = dict(_GOOD, **over)
        assert set(named) <= {n for _, n in params}, what
        full = lib.gsl_map_view_ws_bytes(named["n_rows"])
        args = []
        for c_type, name in params:
            if name == "stream":
                args.append(None)
            elif name in named:
                args.append({"full": full, "short": full - 1}[named[name]] if isinstance(named[name], str)
                            else named[name])
            else:
                args.append(ctypes.addressof(buf) if "*" in c_type else 0)
        assert getattr(lib, FN)(*args) == want, what
    assert not any(buf.raw)  # nothing wrote to the buffer


def test_map_config_validation():
    assert MapConfig().free_rho is None and MapConfig().free_window_px == 1
    assert MapConfig(free_rho=0.05, free_window_px=0).free_window_px == 0
    assert MapConfig(free_rho=0.5, free_window_px=3).free_rho == 0.5
    for kw in (dict(free_rho=0.0), dict(free_rho=1.0), dict(free_rho=-0.1), dict(free_rho=1.5),
               dict(free_rho=float("nan"))):
        with pytest.raises(ValueError, match="free_rho"):
            MapConfig(**kw)
    for kw in (dict(free_window_px=-1), dict(free_window_px=4), dict(free_window_px=1.5), dict(free_window_px=True)):
        with pytest.raises(ValueError, match="free_window_px"):
            MapConfig(**kw)


# ---- GaussianMap.remove_seen_through around the mirror --------------------------------------------------------------
W, H = base.W, base.H
CFG_NEAR = TrackerConfig().gs.near_plane


class _FreeMirrorMap(base._MirrorMap):
    """GaussianMap whose device calls are the numpy mirrors; records the order of its calls and what the removal got."""
    log = []

    def _launch(self, depth, rgb, intr, c2w, render, alphas):
        _FreeMirrorMap.log.append(dict(call="insert"))
        return super()._launch(depth, rgb, intr, c2w, render, alphas)

    def _free_launch(self, depth, intr, w2c, keep, window, near):
        f = self._free_buffers()
        r = ref.select(self.means[:self.n_live].numpy(), w2c.numpy(), intr, depth.numpy(), F32(keep), window, near)
        _FreeMirrorMap.log.append(dict(call="free", depth=depth.clone(), w2c=w2c.numpy().copy(), keep=keep, window=window,
                                       near=near, rows=self.n_live, kept=r["kept"], tested=r["tested"]))
        ids = torch.from_numpy(r["ids"]).long()
        f["means"][:len(ids)], f["colors"][:len(ids)] = self.means[ids], self.colors[ids]
        f["ids"][:len(ids)] = torch.from_numpy(r["ids"])
        return r["counters"][0], r["counters"][2]


def _room_map(config, ghosts=True):
    """A map of the 32x24 room seen from the identity pose; ``ghosts``: the rows of the pixels 10..19 x 8..15 pulled to
    half their distance, in front of the far wall."""
    from gsplatloc_amd.my_gsplat.geometry import depth_to_points

    K = replica_intrinsics(W, H)
    depth = room_depth(W, H, K, torch.eye(4))
    m = _FreeMirrorMap(W, H, config, "cpu")
    m.means[:W * H] = depth_to_points(depth, K)
    m.colors[:W * H] = torch.rand(W * H, 3, generator=torch.Generator().manual_seed(1))
    m.n_live = W * H
    block = torch.zeros(H, W, dtype=torch.bool)
    if ghosts:
        block[8:16, 10:20] = True
        m.means[:W * H][block.reshape(-1)] *= 0.5
    return m, K, depth, block.reshape(-1)


def test_remove_seen_through_swaps_the_buffers_only_when_something_goes():
    cfg = MapConfig(free_rho=0.05, capacity=W * H + 7)
    # the room as it is: nothing is seen through, nothing changes
    m, K, depth, _ = _room_map(cfg, ghosts=False)
    before, ptr, m._view_rows = m.points.clone(), m.means.data_ptr(), m.n_live
    assert m.survivors.numel() == 0
    assert m.remove_seen_through(depth, K, torch.eye(4), CFG_NEAR) == (0, W * H)
    assert m.means.data_ptr() == ptr and m.n_live == W * H == m._view_rows and torch.equal(m.points, before)
    assert torch.equal(m.survivors, torch.arange(W * H, dtype=torch.int32))
    # with ghosts: exactly they go, the others keep their order, the spare pair is the map now
    m, K, depth, block = _room_map(cfg)
    before, colors, ptr, cptr, m._view_rows = m.points.clone(), m.point_colors.clone(), m.means.data_ptr(), \
        m.colors.data_ptr(), m.n_live
    assert m.remove_seen_through(depth, K, torch.eye(4), CFG_NEAR) == (80, W * H - 80)
    assert m.n_live == W * H - 80 and m._view_rows == -1
    assert m.means.data_ptr() != ptr and m.colors.data_ptr() != cptr and m.means.shape == (cfg.capacity, 3)
    assert m._free["means"].data_ptr() == ptr and m._free["colors"].data_ptr() == cptr  # a swap: the old pair is the spare
    assert torch.equal(m.points, before[~block]) and torch.equal(m.point_colors, colors[~block])
    assert m.survivors.dtype == torch.int32 and torch.equal(m.survivors.long(), torch.nonzero(~block).reshape(-1))
    call = _FreeMirrorMap.log[-1]
    assert call["keep"] == float(ref.keep_of(0.05)) and call["window"] == 1 and call["near"] == CFG_NEAR
    assert np.array_equal(call["w2c"], np.eye(4, dtype=F32)) and call["rows"] == W * H
    # a second frame from the same pose removes nothing and swaps nothing back
    ptr = m.means.data_ptr()
    assert m.remove_seen_through(depth, K, torch.eye(4), CFG_NEAR) == (0, W * H - 80) and m.means.data_ptr() == ptr
    # window 0 against window 1 on a depth image with one invalid pixel beside the ghosts
    holed = depth.clone()
    holed[12, 9] = 0.0
    for window, gone in ((0, 80), (1, 77)):  # the three ghosts of column 10, lines 11..13, have it in their window
        m = _room_map(MapConfig(free_rho=0.05, free_window_px=window))[0]
        assert m.remove_seen_through(holed, K, torch.eye(4), CFG_NEAR)[0] == gone
    m.clear()
    assert m.n_live == 0 and m.survivors.numel() == 0
    assert m.remove_seen_through(depth, K, torch.eye(4), CFG_NEAR) == (0, 0)  # an empty map: nothing, no call


def test_a_map_on_the_host_has_no_removal_path():
    m = GaussianMap(W, H, MapConfig(free_rho=0.05), "cpu")
    assert m.remove_seen_through(torch.ones(H, W), replica_intrinsics(W, H), torch.eye(4), CFG_NEAR) == (0, 0)
    m.n_live = 3
    with pytest.raises(AssertionError, match="no CPU path"):
        m.remove_seen_through(torch.ones(H, W), replica_intrinsics(W, H), torch.eye(4), CFG_NEAR)
    with pytest.raises(ValueError, match="depth"):
        m.remove_seen_through(torch.ones(H, W + 1), replica_intrinsics(W, H), torch.eye(4), CFG_NEAR)
    grow_only = GaussianMap(W, H, MapConfig(), "cpu")
    grow_only.n_live = 3
    with pytest.raises(RuntimeError, match="free_rho"):
        grow_only.remove_seen_through(torch.ones(H, W), replica_intrinsics(W, H), torch.eye(4), CFG_NEAR)


# ---- Localizer(mode="map", free_rho) around stand-ins ---------------------------------------------------------------
def _localizer(tracker, renderer, config):
    tracker.made = base._Tracker.made = []
    _FreeMirrorMap.log = []
    return Localizer(replica_intrinsics(W, H), W, H, TrackerConfig(max_steps=5), normalize=False, motion="hold",
                     device="cpu", tracker_factory=tracker, mode="map", map_factory=_FreeMirrorMap, map_renderer=renderer,
                     map_config=config)


def _no_query_render(monkeypatch):
    import gsplatloc_amd.data.dataset as DS

    monkeypatch.setattr(DS, "compute_depth_gt", lambda pts, col, Ks, c2w, height, width: torch.zeros(height, width))


def _add_ghosts(loc):
    """Frame 0 was taken at the identity: halving the rows of a block of its pixels puts them in front of the wall."""
    block = torch.zeros(H, W, dtype=torch.bool)
    block[8:16, 10:20] = True
    loc.map.means[:W * H][block.reshape(-1)] *= 0.5
    return block.reshape(-1)


def test_free_rho_removes_after_the_insertion(sequence, monkeypatch):  # noqa: F811
    _no_query_render(monkeypatch)
    frames = sequence
    loc = _localizer(base._Tracker, base._Renderer(), MapConfig(free_rho=0.05))
    loc.reset(*frames[0])
    ghosts = _add_ghosts(loc)
    _FreeMirrorMap.log = []
    ptr, before = loc.map.means.data_ptr(), loc.map.points.clone()
    loc.map._view_rows = loc.map.n_live
    r = loc.track(frames[1][0], frames[1][1], gt_c2w=frames[1][2])
    # insert first, then remove -- with the frame's depth, the world estimate, the tracker's near plane
    assert [c["call"] for c in _FreeMirrorMap.log] == ["insert", "free"]
    call = _FreeMirrorMap.log[1]
    assert torch.equal(call["depth"], frames[1][0]) and np.array_equal(call["w2c"], ref.w2c_of(r.c2w.numpy()))
    assert call["near"] == CFG_NEAR and call["keep"] == float(ref.keep_of(0.05)) and call["window"] == 1
    assert r.added == H and call["rows"] == W * H + H  # the rows just appended were judged as well ...
    assert call["kept"][W * H:].all() and call["tested"][W * H:].all()  # ... and sit on the observed surface
    # exactly the ghosts went (the stand-in tracker answers the ground truth)
    assert np.array_equal(~call["kept"][:W * H], ghosts.numpy()) and r.removed == 80
    assert r.map_size == W * H + H - 80 == loc.map.n_live and not r.lost
    assert loc.map.means.data_ptr() != ptr and loc.map._view_rows == -1
    assert torch.equal(loc.map.points[:W * H - 80], before[~ghosts])
    assert torch.equal(loc.map.survivors.long()[:W * H - 80], torch.nonzero(~ghosts).reshape(-1))
    # the next frame: nothing left to remove, nothing swapped; the tracker was rebuilt for the new count
    ptr, size = loc.map.means.data_ptr(), loc.map.n_live
    loc.map._view_rows = size
    r2 = loc.track(frames[2][0], frames[2][1], gt_c2w=frames[2][2])
    assert r2.removed == 0 and r2.added == H and r2.map_size == size + H and r2.tracked == size
    assert loc.map.means.data_ptr() == ptr and loc.map._view_rows == size
    assert [t.args[0] for t in base._Tracker.made] == [W * H, size]
    assert [c["call"] for c in _FreeMirrorMap.log] == ["insert", "free", "insert", "free"]


def test_free_rho_a_lost_frame_removes_nothing(sequence):  # noqa: F811
    frames = sequence
    loc = _localizer(base._LostTracker, base._Renderer(), MapConfig(free_rho=0.05))
    loc.reset(*frames[0])
    _add_ghosts(loc)
    _FreeMirrorMap.log = []
    ptr, before = loc.map.means.data_ptr(), loc.map.points.clone()
    r = loc.track(frames[1][0], frames[1][1])
    assert r.lost and r.removed == 0 and r.added == 0 and r.map_size == W * H == loc.map.n_live
    assert _FreeMirrorMap.log == [] and loc.map.means.data_ptr() == ptr and torch.equal(loc.map.points, before)


def test_without_free_rho_nothing_is_removed_and_nothing_changes(sequence, monkeypatch):  # noqa: F811
    """free_rho=None: no removal call even with ghosts in the map, ``removed`` is None, and loads, renders, rows and
    results are those of the map without the method's device call at all (tests/test_map_cpu.py's mirror map)."""
    _no_query_render(monkeypatch)
    runs = []
    for factory in (base._MirrorMap, _FreeMirrorMap):
        renderer = base._Renderer()
        base._Tracker.made = []
        _FreeMirrorMap.log = []
        loc = Localizer(replica_intrinsics(W, H), W, H, TrackerConfig(max_steps=5), normalize=False, motion="hold",
                        device="cpu", tracker_factory=base._Tracker, mode="map", map_factory=factory,
                        map_renderer=renderer, map_config=MapConfig())
        loc.reset(*sequence[0])
        _add_ghosts(loc)
        results = [loc.track(f[0], f[1], gt_c2w=f[2]) for f in sequence[1:4]]
        assert all(c["call"] == "insert" for c in _FreeMirrorMap.log) and loc.map._free is None
        assert all(r.removed is None for r in results)
        assert [(r.added, r.map_size, r.tracked) for r in results] == [(H, W * H + (k + 1) * H, W * H + k * H)
                                                                       for k in range(3)]
        fields = [(r.steps, r.best_step, r.best_loss, r.lost, r.eT, r.eR, r.view_violations) for r in results]
        runs.append((fields, [t.loads[-1] for t in base._Tracker.made], renderer.calls, loc.map.points.clone(),
                     loc.trajectory.clone()))
    (f_a, loads_a, renders_a, points_a, traj_a), (f_b, loads_b, renders_b, points_b, traj_b) = runs
    assert f_a == f_b and len(loads_a) == len(loads_b) == 3
    for a, b in zip(loads_a + renders_a, loads_b + renders_b):
        for name in a:
            assert (a[name] is None and b[name] is None) or torch.equal(a[name], b[name]), name
    assert torch.equal(points_a, points_b) and torch.equal(traj_a, traj_b)


def test_the_options_of_the_evaluation_driver_need_the_map_mode(tmp_path, capsys):
    from gsplatloc_amd import eval as ev

    with pytest.raises(ValueError, match="map_free_rho"):
        ev.evaluate_room(None, 200, 3, sequential=True, map_free_rho=0.05)
    for extra in (["--map-free-rho", "0.05"], ["--sequential", "--map-free-rho", "0.05"], ["--map-free-window", "2"]):
        with pytest.raises(SystemExit):
            ev.main(["--root", str(tmp_path)] + extra)
        assert "needs --map" in capsys.readouterr().err


# ---- the synthetic sequence -----------------------------------------------------------------------------------------
def test_vanishing_panel_sequence(tmp_path):
    from gsplatloc_amd.data import Parser

    w, h = 160, 120
    K = replica_intrinsics(w, h)
    room, panel = room_depth(w, h, K, torch.eye(4)), panel_depth(w, h, K, torch.eye(4))
    on = panel < room
    assert int(on.sum()) == 484 and bool((panel[on] == 1.5).all()) and torch.equal(panel[~on], room[~on])
    rows, cols = torch.nonzero(on.any(1)).reshape(-1), torch.nonzero(on.any(0)).reshape(-1)
    assert len(rows) == len(cols) == 22 and bool(on[rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1].all())  # a rectangle
    # a panel behind the camera, or outside the room's depth, changes nothing
    assert torch.equal(panel_depth(w, h, K, torch.eye(4), z=-1.0), room)
    assert torch.equal(panel_depth(w, h, K, torch.eye(4), z=3.5), room)
    poses = write_replica_vanishing_panel(tmp_path, w, h, 5, 2)
    assert poses.shape == (5, 4, 4) and torch.equal(poses[0], torch.eye(4, dtype=torch.float64))
    parser = Parser("Replica", "room0", normalize=False, device="cpu", input_folder=str(tmp_path))
    for i in range(5):
        depth, _, pose = parser.frame(i)
        want = (panel_depth if i < 2 else room_depth)(w, h, K, poses[i].float())
        assert float((depth - want).abs().max()) <= 0.5 / 6553.5 + 1e-6 and float((pose - poses[i].float()).abs().max()) <= 1e-6
        assert (int((depth < 1.6).sum()) > 400) == (i < 2)


def test_the_existing_writers_write_what_they_wrote(tmp_path):
    """The depth hook of the shared writer leaves the other sequences' files as they were: the same bytes as a writer
    without the hook produces (room_depth of every pose, the image generator seeded with 11)."""
    import hashlib

    from PIL import Image

    from gsplatloc_amd.synthetic import write_replica_constant_twist

    poses = write_replica_constant_twist(tmp_path, 32, 24, 3)
    K = replica_intrinsics(32, 24)
    rng = np.random.default_rng(11)
    for i in range(3):
        depth = room_depth(32, 24, K, poses[i].float()).numpy()
        got = np.array(Image.open(tmp_path / "room0" / "results" / f"depth{i:06d}.png"))
        assert got.dtype == np.uint16 and np.array_equal(got, np.round(depth * 6553.5).astype(np.uint16))
        want = tmp_path / f"want{i}.jpg"
        Image.fromarray(rng.integers(0, 255, (24, 32, 3), dtype=np.uint8)).save(want)
        have = tmp_path / "room0" / "results" / f"frame{i:06d}.jpg"
        assert hashlib.sha256(have.read_bytes()).digest() == hashlib.sha256(want.read_bytes()).digest()


# ---- the kernel's budget --------------------------------------------------------------------------------------------
@pytest.mark.skipif(not __import__("os").path.exists(HIPCC), reason="hipcc not installed")
def test_the_rule_kernel_stays_in_registers():
    """k_map_free_select: no scratch, no accumulation registers, the helper's 16 bytes of LDS, eight waves per SIMD --
    and a name the budget test of the other compactions does not pick up."""
    res = _resources("map_free.hip")
    hit = [v for k, v in res.items() if "k_map_free_select" in k]
    assert len(hit) == 1, list(res)
    r = hit[0]
    assert r["ScratchSize"] == 0 and r["Occupancy"] == 8 and r["AGPRs"] == 0 and r["LDS"] <= 16, r
    assert not any("k_map_select" in k or "k_map_view_select" in k for k in res)
