"""A bounded map (the least recently observed rows are evicted), the parts that need no GPU: the properties of the mirror
tests/map_evict_ref.py on random stamps and its OBSERVED rule on hand-made rows, the argument checks of the entry
points, MapConfig, GaussianMap.observe / evict / insert_frame and Localizer(mode="map") with ``evict`` around the
stand-in tracker / renderer of tests/test_map_cpu.py and a map whose device calls are the mirrors, and the register
budget of the kernels.

The hand-made rows: a 6x4 image, the identity pose, intrinsics (4, 4, 2, 1) -- u = 4 x / z + 2, v = 4 y / z + 1 -- and
dyadic rows and keep = 0.5, so that every product, quotient and sum of the rule is exact."""
import ctypes

import numpy as np
import pytest
import torch

from gsplatloc_amd import _lib
from gsplatloc_amd.localizer import Localizer
from gsplatloc_amd.mapping import GaussianMap, MapConfig
from gsplatloc_amd.my_gsplat import TrackerConfig
from gsplatloc_amd.synthetic import replica_intrinsics
from tests import map_evict_ref as ref
from tests import map_ref
from tests import test_map_cpu as base
from tests.test_abi import prototypes
from tests.test_kernel_resources import HIPCC, _resources
from tests.test_map_cpu import sequence  # noqa: F401  (the 32x24 drifting sequence, a module fixture there)

F32 = np.float32
RW, RH, INTR = 6, 4, (4.0, 4.0, 2.0, 1.0)
EYE = np.eye(4, dtype=F32)
NEAR, FAR = 0.25, 8.0
FLAT = np.full((RH, RW), 2.0, F32)  # a surface at 2 m everywhere


# ---- the mirror of the eviction rule --------------------------------------------------------------------------------
def _patterns(rng, n, now):
    yield "random", rng.integers(now - 40, now + 1, n)
    yield "all equal", np.full(n, now - 3)
    yield "distinct", now - 1 - rng.permutation(n)
    yield "two classes", np.where(rng.random(n) < 0.4, now - 9, now - 2)
    yield "current frame", np.full(n, now)
    yield "clamp", rng.choice([now - 1022, now - 1023, now - 1024, now - 5000, now, now + 7], n)


@pytest.mark.parametrize("n", [1, 7, 64, 257, 1000])
def test_select_properties_on_random_stamps(n):
    rng, now = np.random.default_rng(n), 6000
    for name, stamps in _patterns(rng, n, now):
        stamps = stamps.astype(np.int32)
        age = ref.ages(stamps, now)
        assert age.min() >= 0 and age.max() <= 1023
        for min_age in (1, 3, 1023):
            evictable = int((age >= min_age).sum())
            for need in sorted({0, 1, evictable - 1, evictable, evictable + 1, n + 5} - {-1}):
                r = ref.select(stamps, now, min_age, need)
                what = (name, n, min_age, need)
                gone = ~r["kept"]
                # the evicted count is min(need, evictable), and only evictable rows go
                assert r["E"] == int(gone.sum()) == min(need, evictable) and r["evictable"] == evictable, what
                assert (age[gone] >= min_age).all(), what
                assert r["counters"] == (n - r["E"], r["E"], n - r["E"]) and len(r["ids"]) == n - r["E"], what
                assert np.array_equal(r["ids"], np.flatnonzero(r["kept"])) and r["ids"].dtype == np.int32
                # nothing that stays and could have gone is older than anything that went (ages clamped)
                stay_ev = r["kept"] & (age >= min_age)
                if gone.any() and stay_ev.any():
                    assert age[gone].min() >= age[stay_ev].max(), what
                # ties go in map order: the evicted rows of the threshold age are the first of that age
                ties = np.flatnonzero(age == r["a_star"])
                assert np.array_equal(r["ties"], age == r["a_star"])
                assert np.array_equal(np.flatnonzero(gone & (age == r["a_star"])), ties[:r["quota"]]), what
                assert gone[age > r["a_star"]].all() and not gone[age < r["a_star"]].any(), what
                if need == 0 or evictable == 0:
                    assert r["kept"].all() and (r["a_star"], r["quota"], r["E"]) == (1023, 0, 0), what
                if need > n:
                    assert np.array_equal(gone, age >= min_age), what  # everything that can go goes, nothing else


def test_select_by_hand():
    now = 10
    stamps = np.array([10, 4, 9, 4, 7, 4, 10, -2000], np.int32)  # ages 0 6 1 6 3 6 0 1023
    assert ref.ages(stamps, now).tolist() == [0, 6, 1, 6, 3, 6, 0, 1023]
    r = ref.select(stamps, now, 1, 3)  # the clamped row, then the first two of the three rows of age 6
    assert (r["a_star"], r["quota"], r["E"], r["evictable"]) == (6, 2, 3, 6) and r["ids"].tolist() == [0, 2, 4, 5, 6]
    r = ref.select(stamps, now, 1, 4)  # all of age 6: the quota is the whole class
    assert (r["a_star"], r["quota"]) == (6, 3) and r["ids"].tolist() == [0, 2, 4, 6]
    r = ref.select(stamps, now, 1, 5)
    assert (r["a_star"], r["quota"]) == (3, 1) and r["ids"].tolist() == [0, 2, 6]
    r = ref.select(stamps, now, 1, 100)  # the rows of the current frame never go
    assert (r["a_star"], r["E"]) == (1, 6) and r["ids"].tolist() == [0, 6]
    r = ref.select(stamps, now, 4, 100)  # min_age 4: ages 1 and 3 stay as well
    assert (r["a_star"], r["E"]) == (6, 4) and r["ids"].tolist() == [0, 2, 4, 6]
    r = ref.select(stamps, now, 1, 0)
    assert r["kept"].all() and (r["a_star"], r["quota"], r["E"]) == (1023, 0, 0)
    # stamps from the future and beyond the int32 difference: age 0, no overflow
    far = np.array([2**31 - 1, -2**31], np.int32)
    assert ref.ages(far, -5).tolist() == [0, 1023] and ref.ages(far, 2**31 - 1).tolist() == [0, 1023]


# ---- the mirror of the OBSERVED rule --------------------------------------------------------------------------------
def _p(u, v, z=2.0):
    return [(u - 2.0) / 4.0 * z, (v - 1.0) / 4.0 * z, z]


def _seen(points, depth=FLAT, window=0, keep=0.5, reach=1.0, near=NEAR, far=FAR):
    return ref.observed(np.array(points, F32).reshape(-1, 3), EYE, INTR, depth, F32(keep), window, reach, near,
                        far).tolist()


def test_observed_each_clause_alone():
    # on the surface, and on both thresholds: z == d * keep and z * keep == d
    assert _seen([_p(3, 2, 2.0), _p(3, 2, 1.0), _p(3, 2, 4.0)]) == [True, True, True]
    step = lambda z, to: float(np.nextafter(F32(z), F32(to)))  # noqa: E731
    assert _seen([_p(3, 2, step(1.0, 0)), _p(3, 2, step(4.0, 9))]) == [False, False]
    assert _seen([_p(3, 2, step(1.0, 9)), _p(3, 2, step(4.0, 0))]) == [True, True]
    # a pixel without depth agrees with nothing
    for bad in (0.0, -1.0, np.nan, np.inf, -np.inf):
        d = FLAT.copy()
        d[2, 3] = bad
        assert _seen([_p(3, 2)], d) == [False] and _seen([_p(3, 2)], d, window=1) == [True]
    # the window: only a neighbour shows the row's depth
    d = np.full((RH, RW), 7.5, F32)
    d[1, 1] = 2.0
    assert [_seen([_p(2, 2)], d, w) for w in (0, 1)] == [[False], [True]]
    assert [_seen([_p(3, 3)], d, w) for w in (0, 1, 2)] == [[False], [False], [True]]
    # the reach band: outside the image there is no depth to hold the row against
    assert _seen([_p(-1, 1), _p(RW, 1), _p(2, -1), _p(2, RH)]) == [True] * 4  # u = -1 is -reach, RW is W - 1 + reach
    assert _seen([_p(-1.25, 1), _p(RW + 0.25, 1), _p(2, -1.25), _p(2, RH + 0.25)]) == [False] * 4
    assert _seen([_p(-1, 1, 0.5)], FLAT) == [True]  # ... whatever its depth
    assert _seen([_p(-0.5, 1, 7.0)]) == [False]  # rounds to -0: column 0, inside, and 7 m is not the surface
    assert _seen([_p(-1, 1)], reach=0.5) == [False]
    # the depth planes, and rows that are not numbers
    assert _seen([_p(2, 1, NEAR), _p(2, 1, FAR)], np.full((RH, RW), NEAR, F32), keep=1.0) == [False, False]
    assert _seen([_p(2, 1, step(NEAR, 9))], np.full((RH, RW), step(NEAR, 9), F32), keep=1.0) == [True]
    nan, inf = np.nan, np.inf
    assert _seen([[nan, 0, 2], [0, nan, 2], [0, 0, nan], [inf, 0, 2], [0, 0, inf], [0, 0, -inf], [0, 0, -2.0]]) == [False] * 7
    assert ref.stamp(np.array([5, 6, 7], np.int32), np.array([True, False, True]), 9).tolist() == [9, 6, 9]


# ---- the entry points' argument checks ------------------------------------------------------------------------------
BAD_ARG, WORKSPACE = -1, -2
_OBSERVE = dict(n_rows=1000, fx=50.0, fy=40.0, cx=31.5, cy=23.5, width=64, height=48, keep=0.95, window_px=1,
                reach_px=4.0, near_plane=0.01, far_plane=10.0, now=3)
_SELECT = dict(n_rows=1000, now=9, min_age=1, need=10, ws_bytes="full")
_GATHER = dict(n_src=1000, n_ids=10)
_ROWS = [
    ("gsl_map_observe", _OBSERVE, [
        ("NULL means", dict(means=None)), ("NULL w2c", dict(w2c=None)), ("NULL depth", dict(depth=None)),
        ("NULL stamps", dict(stamps=None)), ("n_rows == 0", dict(n_rows=0)), ("n_rows < 0", dict(n_rows=-5)),
        ("n_rows == 2^31", dict(n_rows=1 << 31)), ("width <= 0", dict(width=0)), ("height <= 0", dict(height=-3)),
        ("2^31 pixels", dict(width=65536, height=32768)), ("fx == 0", dict(fx=0.0)), ("fy == -0", dict(fy=-0.0)),
        ("keep == 0", dict(keep=0.0)), ("keep > 1", dict(keep=1.0000001)), ("NaN keep", dict(keep=float("nan"))),
        ("window < 0", dict(window_px=-1)), ("window > 3", dict(window_px=4)), ("reach < 0", dict(reach_px=-0.5)),
        ("NaN reach", dict(reach_px=float("nan"))), ("near == far", dict(near_plane=10.0)),
        ("near > far", dict(near_plane=11.0)), ("NaN far", dict(far_plane=float("nan")))]),
    ("gsl_map_evict_select", _SELECT, [
        ("NULL stamps", dict(stamps=None)), ("NULL counters", dict(counters=None)), ("NULL ws", dict(ws=None)),
        ("n_rows == 0", dict(n_rows=0)), ("n_rows < 0", dict(n_rows=-1)), ("n_rows == 2^31", dict(n_rows=1 << 31)),
        ("n_rows beyond 2^32", dict(n_rows=(1 << 32) + 7)), ("need < 0", dict(need=-1)), ("min_age == 0", dict(min_age=0)),
        ("min_age < 0", dict(min_age=-4)), ("short workspace", dict(ws_bytes=8), WORKSPACE),
        ("the view's workspace", dict(ws_bytes="view"), WORKSPACE),
        ("workspace one byte short", dict(ws_bytes="short"), WORKSPACE)]),
    ("gsl_map_gather_i32", _GATHER, [
        ("NULL src", dict(src=None)), ("NULL ids", dict(ids=None)), ("NULL dst", dict(dst=None)),
        ("n_src == 0", dict(n_src=0)), ("n_src == 2^31", dict(n_src=1 << 31)), ("n_ids < 0", dict(n_ids=-1)),
        ("n_ids == 2^31", dict(n_ids=1 << 31))]),
]


def test_entry_points_reject_bad_arguments_before_any_launch(repo_root):
    """Every row is refused on the host: the pointers are one dummy HOST buffer, a launch would give GSL_ERR_HIP or
    worse."""
    lib = _lib.load_library()
    protos = prototypes(repo_root)
    assert [n for _, n in protos["gsl_map_observe"][1]] == [
        "means", "n_rows", "w2c", "fx", "fy", "cx", "cy", "depth", "width", "height", "keep", "window_px", "reach_px",
        "near_plane", "far_plane", "now", "stamps", "stream"]
    assert [n for _, n in protos["gsl_map_evict_select"][1]] == [
        "stamps", "n_rows", "now", "min_age", "need", "counters", "ws", "ws_bytes", "stream"]
    assert [n for _, n in protos["gsl_map_gather_i32"][1]] == ["src", "n_src", "ids", "n_ids", "dst", "stream"]
    buf = ctypes.create_string_buffer(256)
    for fn, good, rows in _ROWS:
        params = protos[fn][1]
        for what, over, *want in rows:
            named = dict(good, **over)
            assert set(named) <= {n for _, n in params}, (fn, what)
            sizes = {}
            if "n_rows" in named and fn == "gsl_map_evict_select":
                full = lib.gsl_map_evict_ws_bytes(named["n_rows"])
                sizes = {"full": full, "short": full - 1, "view": lib.gsl_map_view_ws_bytes(named["n_rows"])}
            args = []
            for c_type, name in params:
                if name == "stream":
                    args.append(None)
                elif name in named:
                    args.append(sizes[named[name]] if isinstance(named[name], str) else named[name])
                else:
                    args.append(ctypes.addressof(buf) if "*" in c_type else 0)
            assert getattr(lib, fn)(*args) == (want[0] if want else BAD_ARG), (fn, what)
    assert lib.gsl_map_gather_i32(ctypes.addressof(buf), 5, ctypes.addressof(buf), 0, ctypes.addressof(buf), None) == 0
    assert not any(buf.raw)  # nothing wrote to the buffer


def test_workspace_size():
    """The head is the local map's workspace; behind it the tie ballots, 1024 bins and four parameters."""
    lib = _lib.load_library()
    for n in (1, 256, 257, 4099, 375000, (1 << 31) - 1):
        nb = (n + 255) // 256
        assert lib.gsl_map_view_ws_bytes(n) == 48 * nb
        assert lib.gsl_map_evict_ws_bytes(n) == 48 * nb + 32 * nb + 4 * 1024 + 16


def test_map_config_validation():
    c = MapConfig()
    assert (c.evict, c.evict_min_age, c.evict_headroom, c.observe_window_px) == (False, 1, 0, 1)
    c = MapConfig(evict=True, evict_min_age=5, evict_headroom=100, observe_window_px=3)
    assert (c.evict, c.evict_min_age, c.evict_headroom, c.observe_window_px) == (True, 5, 100, 3)
    for kw, word in ((dict(evict=1), "evict"), (dict(evict=None), "evict"), (dict(evict_min_age=0), "evict_min_age"),
                     (dict(evict_min_age=-1), "evict_min_age"), (dict(evict_min_age=1.5), "evict_min_age"),
                     (dict(evict_min_age=True), "evict_min_age"), (dict(evict_min_age=1024), "evict_min_age"),
                     (dict(evict_headroom=-1), "evict_headroom"), (dict(evict_headroom=0.5), "evict_headroom"),
                     (dict(observe_window_px=-1), "observe_window_px"), (dict(observe_window_px=4), "observe_window_px"),
                     (dict(observe_window_px=1.0), "observe_window_px"), (dict(evict=True, depth_rho=1.0), "depth_rho")):
        with pytest.raises(ValueError, match=word):
            MapConfig(**kw)


# ---- GaussianMap around the mirrors ---------------------------------------------------------------------------------
W, H = base.W, base.H
CFG_NEAR, CFG_FAR = TrackerConfig().gs.near_plane, TrackerConfig().gs.far_plane


class _EvictMirrorMap(base._MirrorMap):
    """GaussianMap whose device calls are the numpy mirrors; records the order of its calls."""
    log = []

    def _launch(self, depth, rgb, intr, c2w, render, alphas):
        _EvictMirrorMap.log.append(dict(call="insert", rows=self.n_live, now=self.frame_index))
        return super()._launch(depth, rgb, intr, c2w, render, alphas)

    def _select_launch(self, depth, render, alphas):
        sel = map_ref.select(depth.numpy(), None if render is None else render.numpy(),
                             None if alphas is None else alphas.numpy(), self.alpha_min, F32(self.keep))
        _EvictMirrorMap.log.append(dict(call="select", rows=self.n_live, selected=int(sel.sum())))
        self._pending = (render, alphas)
        return int(sel.sum())

    def _append_launch(self, depth, rgb, intr, c2w):
        _EvictMirrorMap.log.append(dict(call="append", rows=self.n_live, now=self.frame_index))
        return base._MirrorMap._launch(self, depth, rgb, intr, c2w, *self._pending)[1]

    def _observe_launch(self, depth, intr, w2c, near, far):
        seen = ref.observed(self.means[:self.n_live].numpy(), w2c.numpy(), intr, depth.numpy(), F32(self.keep),
                            self.cfg.observe_window_px, self.cfg.view_reach_px, near, far)
        _EvictMirrorMap.log.append(dict(call="observe", rows=self.n_live, now=self.frame_index, seen=seen,
                                        w2c=w2c.numpy().copy(), depth=depth.clone(), near=near, far=far))
        self.stamps[:self.n_live] = torch.from_numpy(ref.stamp(self.stamps[:self.n_live].numpy(), seen,
                                                                self.frame_index))

    def _evict_launch(self, need):
        f = self._free_buffers()
        r = ref.select(self.stamps[:self.n_live].numpy(), self.frame_index, self.cfg.evict_min_age, need)
        _EvictMirrorMap.log.append(dict(call="evict", rows=self.n_live, need=need, now=self.frame_index, want=r))
        ids = torch.from_numpy(r["ids"]).long()
        f["means"][:len(ids)], f["colors"][:len(ids)] = self.means[ids], self.colors[ids]
        f["stamps"][:len(ids)], f["ids"][:len(ids)] = self.stamps[ids], torch.from_numpy(r["ids"])
        return r["counters"]


def _filled(config, stamps):
    m = _EvictMirrorMap(W, H, config, "cpu")
    n = len(stamps)
    g = torch.Generator().manual_seed(3)
    m.means[:n], m.colors[:n] = torch.rand(n, 3, generator=g), torch.rand(n, 3, generator=g)
    m.stamps[:n], m.n_live = torch.tensor(stamps, dtype=torch.int32), n
    return m


def test_evict_swaps_the_buffers_and_the_stamps_follow():
    stamps = [5, 1, 4, 1, 3, 1, 5, 2]
    m = _filled(MapConfig(evict=True, capacity=12), stamps)
    m.frame_index, m._view_rows = 5, 8
    means, colors, ptr, sptr = m.points.clone(), m.point_colors.clone(), m.means.data_ptr(), m.stamps.data_ptr()
    assert m.evict(0) == (0, 8) and m.evict(-3) == (0, 8) and m._free is None  # nothing asked for: no call
    keep = [0, 2, 4, 5, 6, 7]  # of the three rows of stamp 1 the first two go
    assert m.evict(2) == (2, 6) and m.n_live == 6 and m._view_rows == -1
    assert m.means.data_ptr() != ptr and m.stamps.data_ptr() != sptr and m._free["means"].data_ptr() == ptr
    assert torch.equal(m.points, means[keep]) and torch.equal(m.point_colors, colors[keep])
    assert m.stamps[:6].tolist() == [stamps[i] for i in keep] and m.survivors.tolist() == keep
    assert m.stamps.shape == (12,) and m.stamps.dtype == torch.int32
    # the rows of the current frame never go: 4 evictable rows are left, 100 are asked for
    assert m.evict(100) == (4, 2) and m.stamps[:2].tolist() == [5, 5] and m.survivors.tolist() == [0, 4]
    ptr = m.means.data_ptr()
    assert m.evict(1) == (0, 2) and m.means.data_ptr() == ptr  # nothing evictable: nothing swapped
    m.clear()
    assert (m.n_live, m.frame_index, m.last_evicted) == (0, 0, 0) and m.evict(5) == (0, 0)
    host = GaussianMap(W, H, MapConfig(evict=True), "cpu")
    host.n_live = 3
    with pytest.raises(AssertionError, match="no CPU path"):
        host.evict(1)
    with pytest.raises(AssertionError, match="no CPU path"):
        host.observe(torch.ones(H, W), replica_intrinsics(W, H), torch.eye(4), 0.1, 9.0)
    assert host.frame_index == 1


def _frame(value=2.0):
    return torch.full((H, W), value), torch.full((H, W, 3), 100.0), replica_intrinsics(W, H), torch.eye(4)


def test_insert_frame_evicts_exactly_what_is_short():
    cap = W * H + 40
    old = [1] * 30 + [2] * 30 + [3] * 30  # frame 3 is the current one
    for headroom in (0, 7):
        _EvictMirrorMap.log = []
        m = _filled(MapConfig(evict=True, capacity=cap, evict_headroom=headroom), old)
        m.frame_index = 3
        means = m.points.clone()
        depth, rgb, K, pose = _frame()
        selected, appended = m.insert_frame(depth, rgb, K, pose)  # no render: every pixel, W * H rows, room for W * H - 50
        short = 50 + headroom
        assert (selected, appended) == (W * H, W * H) and not m.full and m.last_evicted == short
        assert [c["call"] for c in _EvictMirrorMap.log] == ["select", "evict", "append"]
        assert _EvictMirrorMap.log[1]["need"] == short and _EvictMirrorMap.log[2]["rows"] == 90 - short
        assert m.n_live == cap - headroom
        # stamp 1 went whole, of stamp 2 the first rows in map order; the rows appended carry the frame's index
        left = 90 - short
        assert m.stamps[:left].tolist() == [2] * (left - 30) + [3] * 30 and torch.equal(m.points[:left], means[90 - left:])
        assert (m.stamps[left:m.n_live] == 3).all()
    # not enough rows old enough: everything that can go goes, the rest of the frame is dropped
    m = _filled(MapConfig(evict=True, capacity=cap, evict_min_age=2), old)
    m.frame_index = 3
    selected, appended = m.insert_frame(*_frame())
    assert m.last_evicted == 30 and (selected, appended) == (W * H, cap - 60) and m.full and m.n_live == cap
    # without the option the same call drops rows, evicts nothing and asks once
    _EvictMirrorMap.log = []
    m = _filled(MapConfig(capacity=cap), old)
    m.frame_index = 3
    selected, appended = m.insert_frame(*_frame())
    assert (selected, appended) == (W * H, cap - 90) and m.full and m.last_evicted == 0 and m._free is None
    assert [c["call"] for c in _EvictMirrorMap.log] == ["insert"]
    # with the option and room for a whole frame: the single call as well
    _EvictMirrorMap.log = []
    m = _filled(MapConfig(evict=True, capacity=W * H + 90), old)
    assert m.insert_frame(*_frame()) == (W * H, W * H) and not m.full
    assert [c["call"] for c in _EvictMirrorMap.log] == ["insert"] and (m.stamps[90:m.n_live] == 0).all()
    # short of a whole frame but not of this one: the count is read, nothing is evicted
    _EvictMirrorMap.log = []
    m = _filled(MapConfig(evict=True, capacity=cap), old)
    depth = _frame()[0]
    depth[1:] = 0.0  # W pixels with depth
    assert m.insert_frame(depth, *_frame()[1:]) == (W, W) and m.last_evicted == 0 and not m.full
    assert [c["call"] for c in _EvictMirrorMap.log] == ["select", "append"]


# ---- Localizer(mode="map", evict) around stand-ins ------------------------------------------------------------------
def _localizer(tracker, config):
    tracker.made = base._Tracker.made = []
    _EvictMirrorMap.log = []
    return Localizer(replica_intrinsics(W, H), W, H, TrackerConfig(max_steps=5), normalize=False, motion="hold",
                     device="cpu", tracker_factory=tracker, mode="map", map_factory=_EvictMirrorMap,
                     map_renderer=base._Renderer(), map_config=config)


def test_the_localizer_observes_before_it_inserts(sequence, monkeypatch):  # noqa: F811
    import gsplatloc_amd.data.dataset as DS

    monkeypatch.setattr(DS, "compute_depth_gt", lambda pts, col, Ks, c2w, height, width: torch.zeros(height, width))
    frames = sequence
    cap = W * H + H + 5  # frame 1's column fits, frame 2's is 19 rows short
    loc = _localizer(base._Tracker, MapConfig(evict=True, capacity=cap))
    loc.reset(*frames[0])
    assert loc.map.frame_index == 0 and (loc.map.stamps[:W * H] == 0).all()
    assert [c["call"] for c in _EvictMirrorMap.log] == ["insert"]
    loc.map.means[100:140] *= -1.0  # forty rows behind the camera: no later frame observes them
    _EvictMirrorMap.log = []
    r1 = loc.track(frames[1][0], frames[1][1], gt_c2w=frames[1][2])
    log = _EvictMirrorMap.log
    assert [c["call"] for c in log] == ["observe", "select", "append"]
    seen = log[0]
    assert seen["now"] == 1 and seen["rows"] == W * H and torch.equal(seen["depth"], frames[1][0])
    assert np.array_equal(seen["w2c"], ref.w2c_of(r1.c2w.numpy())) and (seen["near"], seen["far"]) == (CFG_NEAR, CFG_FAR)
    assert not seen["seen"][100:140].any() and seen["seen"].sum() > W * H // 2
    assert (r1.added, r1.evicted, r1.map_size) == (H, 0, W * H + H) and not loc.map.full
    assert np.array_equal(loc.map.stamps[:W * H].numpy() == 1, seen["seen"]) and (loc.map.stamps[W * H:W * H + H] == 1).all()
    _EvictMirrorMap.log = []
    r2 = loc.track(frames[2][0], frames[2][1], gt_c2w=frames[2][2])
    log = _EvictMirrorMap.log
    assert [c["call"] for c in log] == ["observe", "select", "evict", "append"]
    assert log[0]["now"] == log[2]["now"] == 2 and log[2]["need"] == H - 5 and log[1]["selected"] == H
    want = log[2]["want"]
    assert want["evictable"] >= H - 5 and want["E"] == H - 5  # the case is what it says: enough rows were not seen
    assert (r2.added, r2.evicted, r2.map_size) == (H, H - 5, cap) and not loc.map.full and loc.map.n_live == cap
    assert (loc.map.stamps[cap - H:cap] == 2).all() and int((loc.map.stamps[:cap] == 2).sum()) >= H
    # the rows that went were the least recently observed of the map before this frame
    assert not want["kept"][ref.ages(loc.map._free["stamps"][:W * H + H].numpy(), 2) > want["a_star"]].any()
    assert [t.args[0] for t in base._Tracker.made] == [W * H, W * H + H]


def test_a_lost_frame_stamps_evicts_and_inserts_nothing(sequence):  # noqa: F811
    frames = sequence
    loc = _localizer(base._LostTracker, MapConfig(evict=True, capacity=W * H + 5))
    loc.reset(*frames[0])
    _EvictMirrorMap.log = []
    r = loc.track(frames[1][0], frames[1][1])
    assert r.lost and (r.added, r.evicted, r.map_size) == (0, 0, W * H)
    assert _EvictMirrorMap.log == [] and loc.map.frame_index == 0 and (loc.map.stamps == 0).all()


def test_without_evict_the_localizer_never_observes(sequence, monkeypatch):  # noqa: F811
    import gsplatloc_amd.data.dataset as DS

    monkeypatch.setattr(DS, "compute_depth_gt", lambda pts, col, Ks, c2w, height, width: torch.zeros(height, width))
    loc = _localizer(base._Tracker, MapConfig(capacity=W * H + H + 5))
    loc.reset(*sequence[0])
    results = [loc.track(f[0], f[1], gt_c2w=f[2]) for f in sequence[1:3]]
    assert [c["call"] for c in _EvictMirrorMap.log] == ["insert"] * 3 and loc.map.frame_index == 0
    assert [(r.added, r.evicted) for r in results] == [(H, None), (5, None)] and loc.map.full


def test_the_option_of_the_evaluation_driver_needs_the_map_mode(tmp_path, capsys):
    from gsplatloc_amd import eval as ev

    with pytest.raises(ValueError, match="map_evict"):
        ev.evaluate_room(None, 200, 3, sequential=True, map_evict=True)
    for extra in (["--map-evict"], ["--sequential", "--map-evict"]):
        with pytest.raises(SystemExit):
            ev.main(["--root", str(tmp_path)] + extra)
        assert "needs --map" in capsys.readouterr().err


# ---- the kernels' budget --------------------------------------------------------------------------------------------
@pytest.mark.skipif(not __import__("os").path.exists(HIPCC), reason="hipcc not installed")
def test_the_kernels_stay_in_registers():
    """No scratch, no accumulation registers, eight waves per SIMD; LDS: the histogram's 4 KB, the threshold's partial
    sums, the compaction helper's 16 bytes, none for the rule and the gather."""
    res = _resources("map_evict.hip")
    lds = {"k_map_observe": 0, "k_map_age_hist": 4096, "k_map_age_threshold": 1028, "k_map_age_ties": 16,
           "k_map_evict_select": 16, "k_map_gather_i32": 0}
    for name, limit in lds.items():
        hit = [v for k, v in res.items() if name in k]
        assert len(hit) == 1, (name, list(res))
        r = hit[0]
        assert r["ScratchSize"] == 0 and r["Occupancy"] == 8 and r["AGPRs"] == 0 and r["LDS"] <= limit, (name, r)
    assert len(res) == len(lds)
