"""GPU: gsl_map_evict_select (csrc/map_evict.hip) followed by gsl_map_view_gather and gsl_map_gather_i32, and
gsl_map_observe, against the numpy mirror tests/map_evict_ref.py on given arrays; GaussianMap.evict / insert_frame /
remove_seen_through with stamps.

Row counts: 1; 63 / 64 / 65 around one wave; 255 / 256 / 257 around one workgroup; 1000; 4099 (17 workgroup counts, three
rows in the last, three workgroups of the histogram).  Stamp patterns: all equal (the tie-break alone decides), all
distinct, two classes, every row of the current frame (nothing evictable), ages 1022 / 1023 / 1024 / 5000 (the clamp and
the last bin), only lane 0 / only lane 63 of every wave old, only the last row old, random.  need: 0, 1, the size of the
oldest class - 1 / + 0 / + 1, evictable - 1, evictable, n + 5.  min_age 1, and 3 on the random pattern.

Every case asserts: the counters after each call; the ballots of the rows that stay and of the rows of age a*; a*, the
tie quota, E and the tie count; out_ids strictly ascending and the mirror's; means / colours / stamps bit copies of the
rows at those ids; the sentinel rows past the count, a guard region behind the outputs and the bytes behind the
workspace untouched; stamps, means and colours unchanged.  Integers only: everything is compared for equality.

gsl_map_observe: the pose, intrinsics and depth image of tests/test_gpu_map_free.py (exact float32 arithmetic, keep =
0.9375), a cloud scattered around the observed surface with hand-made rows on both thresholds (z == d * keep,
z * keep == d), one float32 step off each, on the edge of the reach band and a step outside it, on the depth planes and
NaN / inf rows; windows 0 .. 3.  The stamps must be the mirror's, rows that are not observed keep a sentinel stamp."""
import numpy as np
import pytest
import torch

from gsplatloc_amd import _lib
from gsplatloc_amd.mapping import GaussianMap, MapConfig
from tests import map_evict_ref as ref
from tests import map_free_ref as free_ref
from tests.test_gpu_map_free import EKEEP, _case as _free_case, _exact_depth
from tests.test_gpu_map_view import EH, EINTR, EW, GUARD_ROWS, H, INTR, SENTINEL, W, _exact_pose, _pose, _world

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
ROWS = [1, 63, 64, 65, 255, 256, 257, 1000, 4099]
PATTERNS = ["all_equal", "distinct", "two_classes", "current", "clamp", "lane0", "lane63", "last", "random"]
NOW = 7000
NEAR, FAR, REACH = 0.5, 6.0, 4.0


def _stamps(n, pattern):
    rng = np.random.default_rng(100 * n + len(pattern))
    i = np.arange(n)
    old = {"lane0": i % 64 == 0, "lane63": i % 64 == 63, "last": i == n - 1}
    if pattern in old:
        s = np.where(old[pattern], NOW - 11, NOW)
    else:
        s = {"all_equal": lambda: np.full(n, NOW - 3), "distinct": lambda: NOW - 1 - rng.permutation(n),
             "two_classes": lambda: np.where(rng.random(n) < 0.4, NOW - 9, NOW - 2), "current": lambda: np.full(n, NOW),
             "clamp": lambda: NOW - rng.choice([1022, 1023, 1024, 5000], n),
             "random": lambda: rng.integers(NOW - 40, NOW + 2, n)}[pattern]()
    return s.astype(np.int32)


def _needs(stamps, min_age):
    age = ref.ages(stamps, NOW)
    n, evictable = len(age), int((age >= min_age).sum())
    oldest = int((age == age.max()).sum())
    return sorted({0, 1, oldest - 1, oldest, oldest + 1, evictable - 1, evictable, n + 5} - {-1})


def _bits(words, n):
    bits = ((words[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool).reshape(-1)
    assert not bits[n:].any()  # lanes past the last row hold nothing
    return bits[:n]


def _run(stamps, means, colors, min_age, need):
    """The three entry points on outputs of n + 3 + GUARD_ROWS sentinel rows; everything that was written, on the host."""
    lib, ptr, st = _lib.load_library(), _lib.ptr, _lib.current_stream()
    n = len(stamps)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    s_t, m_t, c_t = t(stamps), t(means), t(colors)
    rows = n + 3 + GUARD_ROWS
    out_m = torch.full((rows, 3), SENTINEL, device=DEV)
    out_c = torch.full((rows, 3), SENTINEL, device=DEV)
    out_i = torch.full((rows,), -77, dtype=torch.int32, device=DEV)
    out_s = torch.full((rows,), -88, dtype=torch.int32, device=DEV)
    counters = torch.full((3,), -5, dtype=torch.int32, device=DEV)
    ws_bytes = lib.gsl_map_evict_ws_bytes(n)
    ws = torch.full((ws_bytes + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    _lib.check(lib.gsl_map_evict_select(ptr(s_t), n, NOW, min_age, need, ptr(counters), ptr(ws), ws_bytes, st),
               "gsl_map_evict_select")
    first = counters.tolist()
    _lib.check(lib.gsl_map_view_gather(ptr(m_t), ptr(c_t), n, ptr(out_m), ptr(out_c), ptr(out_i), n + 3, ptr(counters),
                                       ptr(ws), ws_bytes, st), "gsl_map_view_gather")
    second = counters.tolist()
    _lib.check(lib.gsl_map_gather_i32(ptr(s_t), n, ptr(out_i), second[2], ptr(out_s), st), "gsl_map_gather_i32")
    torch.cuda.synchronize()
    assert bool((ws[ws_bytes:] == 0xAB).all())  # nothing behind the size the library asked for
    for dev, host in ((s_t, stamps), (m_t, means), (c_t, colors)):  # the inputs are only read
        assert np.array_equal(dev.cpu().numpy().view(np.uint32), np.ascontiguousarray(host).view(np.uint32))
    nb = (n + 255) // 256
    raw = ws[:ws_bytes].cpu().numpy()
    assert ws_bytes == 80 * nb + 4096 + 16
    params = raw[80 * nb + 4096:].view(np.uint32).tolist()
    return dict(first=first, counters=second, kept=_bits(raw[:32 * nb].view(np.uint64), n),
                ties=_bits(raw[48 * nb:80 * nb].view(np.uint64), n), bins=raw[80 * nb:80 * nb + 4096].view(np.uint32),
                params=params, ids=out_i.cpu().numpy(), means=out_m.cpu().numpy(), colors=out_c.cpu().numpy(),
                stamps=out_s.cpu().numpy())


def _check(got, want, stamps, means, colors):
    n, k = len(stamps), len(want["ids"])
    assert got["first"] == [k, want["E"], 0]  # after the selection: the rows that stay, E, nothing gathered
    assert tuple(got["counters"]) == want["counters"] == (k, want["E"], k)
    assert np.array_equal(got["kept"], want["kept"]) and np.array_equal(got["ties"], want["ties"])
    assert got["params"] == [want["a_star"], want["quota"], want["E"], int(want["ties"].sum())]
    assert np.array_equal(got["bins"], np.bincount(ref.ages(stamps, NOW), minlength=1024))
    assert np.array_equal(got["ids"][:k], want["ids"]) and (np.diff(got["ids"][:k]) > 0).all()
    assert np.array_equal(got["means"][:k].view(np.uint32), means[want["ids"]].view(np.uint32))
    assert np.array_equal(got["colors"][:k].view(np.uint32), colors[want["ids"]].view(np.uint32))
    assert np.array_equal(got["stamps"][:k], stamps[want["ids"]])
    assert (got["ids"][k:] == -77).all() and (got["stamps"][k:] == -88).all()
    assert (got["means"][k:] == SENTINEL).all() and (got["colors"][k:] == SENTINEL).all()
    assert got["ids"].shape[0] == n + 3 + GUARD_ROWS


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", ROWS)
def test_select_and_gather_against_the_mirror(n, pattern):
    stamps = _stamps(n, pattern)
    rng = np.random.default_rng(n)
    means, colors = rng.normal(size=(n, 3)).astype(F32), rng.uniform(0.0, 1.0, (n, 3)).astype(F32)
    for min_age in (1, 3) if pattern == "random" else (1,):
        for need in _needs(stamps, min_age):
            want = ref.select(stamps, NOW, min_age, need)
            if pattern == "current":
                assert want["E"] == 0 and want["kept"].all()  # the case is what it says
            _check(_run(stamps, means, colors, min_age, need), want, stamps, means, colors)


# ---- gsl_map_observe ------------------------------------------------------------------------------------------------
def _specials():
    """Hand-made rows in the camera frame of the exact pose (u = 64 x / z + 32, v = 64 y / z + 24), and what the rule says
    of them with window 0: (rows [16,3], observed [16]).  The depth image is 2 m in the patch around (7, 7), a float32
    step more in the patch around (19, 7) and 3.75 m at (32, 40): 2 * 0.9375 = 1.875 and 4 * 0.9375 = 3.75 are exact."""
    at = lambda u, v, z: [(u - 32.0) / 64.0 * z, (v - 24.0) / 64.0 * z, z]  # noqa: E731
    step = lambda z, to: float(np.nextafter(F32(z), F32(to)))  # noqa: E731
    rows = [at(7, 7, 1.875),  # z == d * keep: observed
            at(19, 7, 1.875),  # the patch a float32 step deeper: d * keep is one step above z, not observed
            at(32, 40, 4.0),  # z * keep == d: observed
            at(32, 40, step(4.0, 9)),  # a step behind that: not (window 0; a neighbour is deeper)
            at(7, 7, 2.0),  # on the surface
            at(-REACH, 20, 1.0), at(EW - 1 + REACH, 20, 1.0), at(20, -REACH, 1.0), at(20, EH - 1 + REACH, 1.0),  # the band's edge
            at(-REACH - 2.0 ** -17, 20, 1.0), at(20, EH - 1 + REACH + 2.0 ** -17, 1.0),  # a step outside it
            at(-0.5, 20, 1.0),  # rounds to -0: column 0, inside, 1 m is not the surface there
            at(32, 24, NEAR), at(32, 24, FAR),  # on the depth planes
            [np.nan, 0.0, 1.0], [0.0, 0.0, np.inf]]
    seen = [True, False, True, False, True, True, True, True, True, False, False, False, False, False, False, False]
    return np.array(rows), np.array(seen)


def _observe_case(n):
    """A cloud around the surface the exact depth image shows from the exact pose -- most rows within 15 % of the depth
    of their pixel, some in the band around the image -- with the hand-made rows at ``where``."""
    rng = np.random.default_rng(100 * n + 3)
    depth = _exact_depth()
    u, v = rng.uniform(-6.0, EW + 5.0, n), rng.uniform(-6.0, EH + 5.0, n)
    ui, vi = np.clip(np.rint(u), 0, EW - 1).astype(int), np.clip(np.rint(v), 0, EH - 1).astype(int)
    d = depth[vi, ui].astype(np.float64)
    d = np.where(np.isfinite(d) & (d > 0), d, 3.0)
    z = d * rng.uniform(0.85, 1.15, n)
    p = np.stack([(u - 32.0) / 64.0 * z, (v - 24.0) / 64.0 * z, z], axis=-1)
    rows, _ = _specials()
    where = rng.permutation(n)[:min(n, len(rows))]
    p[where] = rows[:len(where)]
    with np.errstate(invalid="ignore"):
        return _world(p, _exact_pose()), where


def _observe(means, w2c, intr, depth, keep, window, now):
    lib, ptr, st = _lib.load_library(), _lib.ptr, _lib.current_stream()
    n, (h, w) = means.shape[0], depth.shape
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    m_t, w_t, d_t = t(means), t(w2c), t(depth)
    stamps = torch.full((n + GUARD_ROWS,), -9, dtype=torch.int32, device=DEV)
    _lib.check(lib.gsl_map_observe(ptr(m_t), n, ptr(w_t), *intr, ptr(d_t), w, h, float(keep), window, REACH, NEAR, FAR,
                                   now, ptr(stamps), st), "gsl_map_observe")
    torch.cuda.synchronize()
    for dev, host in ((m_t, means), (d_t, depth)):
        assert np.array_equal(dev.cpu().numpy().view(np.uint32), np.ascontiguousarray(host).view(np.uint32))
    out = stamps.cpu().numpy()
    assert (out[n:] == -9).all()
    return out[:n]


@pytest.mark.parametrize("window", [0, 1, 2, 3])
@pytest.mark.parametrize("n", ROWS)
def test_observe_against_the_mirror(n, window):
    means, where = _observe_case(n)
    w2c, depth = ref.w2c_of(_exact_pose()), _exact_depth()
    seen = ref.observed(means, w2c, EINTR, depth, EKEEP, window, REACH, NEAR, FAR)
    if n == 4099:
        assert 0.1 <= seen.mean() <= 0.9, seen.mean()
        want = _specials()[1].copy()
        if window >= 1:
            want[3] = True  # the pixel beside (32, 40) is deeper: the row a step behind agrees with it
        assert seen[where].tolist() == want.tolist()
    got = _observe(means, w2c, EINTR, depth, EKEEP, window, 41)
    assert np.array_equal(got, ref.stamp(np.full(n, -9, np.int32), seen, 41))


def test_observe_under_a_general_pose():
    """160x120, the general pose: the rows of a surface at 3 .. 3.1 m are observed, the rows in front of it are not."""
    n = 1000
    means, c2w, intr, depth, _, stays = _free_case(n, "every_other")
    keep = ref.keep_of(0.05)
    seen = ref.observed(means, ref.w2c_of(c2w), intr, depth, keep, 1, REACH, NEAR, FAR)
    assert not seen[~stays].any()  # 1 .. 2 m in front of 3 m
    got = _observe(means, ref.w2c_of(c2w), intr, depth, keep, 1, 5)
    assert np.array_equal(got, ref.stamp(np.full(n, -9, np.int32), seen, 5))


# ---- GaussianMap ----------------------------------------------------------------------------------------------------
def _filled(cap, n, stamps, **cfg):
    rng = np.random.default_rng(n)
    means, colors = rng.normal(size=(n, 3)).astype(F32), rng.uniform(0.0, 1.0, (n, 3)).astype(F32)
    m = GaussianMap(W, H, MapConfig(capacity=cap, **cfg), DEV)
    m.means[:n], m.colors[:n], m.n_live = torch.from_numpy(means).to(DEV), torch.from_numpy(colors).to(DEV), n
    m.stamps[:n] = torch.from_numpy(stamps).to(DEV)
    return m, means, colors


def test_a_map_at_its_capacity_evicts_what_the_mirror_says():
    cap = 30000
    stamps = np.random.default_rng(9).integers(0, 6, cap).astype(np.int32)
    K = torch.tensor([[INTR[0], 0.0, INTR[2]], [0.0, INTR[1], INTR[3]], [0.0, 0.0, 1.0]])
    depth, rgb = torch.full((H, W), 2.0), torch.full((H, W, 3), 100.0)
    depth[0, :7] = 0.0  # seven pixels without depth: W * H - 7 rows are new
    new = W * H - 7
    m, means, colors = _filled(cap, cap, stamps, evict=True)
    m.frame_index = 6
    want = ref.select(stamps, 6, 1, new)
    assert want["E"] == new and 0 < want["quota"] < want["ties"].sum()  # the tie-break decides inside a class
    assert m.insert_frame(depth, rgb, K, torch.eye(4)) == (new, new)
    assert not m.full and m.last_evicted == new and m.n_live == cap
    k = cap - new
    assert np.array_equal(m.survivors.cpu().numpy(), want["ids"])
    assert np.array_equal(m.points[:k].cpu().numpy().view(np.uint32), means[want["ids"]].view(np.uint32))
    assert np.array_equal(m.point_colors[:k].cpu().numpy().view(np.uint32), colors[want["ids"]].view(np.uint32))
    assert np.array_equal(m.stamps[:k].cpu().numpy(), stamps[want["ids"]]) and bool((m.stamps[k:] == 6).all())
    assert bool((m.points[k:, 2] == 2.0).all())  # the frame's rows, at the identity
    # headroom: that many rows more go, and the map ends that far below its capacity
    m, _, _ = _filled(cap, cap, stamps, evict=True, evict_headroom=100)
    m.frame_index = 6
    assert m.insert_frame(depth, rgb, K, torch.eye(4)) == (new, new) and m.last_evicted == new + 100
    assert m.n_live == cap - 100 and not m.full
    # without the option the same call drops the frame
    m, _, _ = _filled(cap, cap, stamps)
    m.frame_index = 6
    assert m.insert_frame(depth, rgb, K, torch.eye(4)) == (new, 0) and m.full and m.last_evicted == 0 and m.n_live == cap


def test_the_stamps_follow_a_removal_of_every_other_row():
    n, cap = 1000, 1500
    K = torch.tensor([[INTR[0], 0.0, INTR[2]], [0.0, INTR[1], INTR[3]], [0.0, 0.0, 1.0]])
    intr = tuple(float(F32(a)) for a in INTR)
    means, c2w, _, depth, _, stays = _free_case(n, "every_other")
    m = GaussianMap(W, H, MapConfig(capacity=cap, free_rho=0.05), DEV)
    m.means[:n], m.n_live = torch.from_numpy(means).to(DEV), n
    stamps = (np.arange(n) * 7 % 1013).astype(np.int32)
    m.stamps[:n] = torch.from_numpy(stamps).to(DEV)
    want = free_ref.select(means, free_ref.w2c_of(c2w), intr, depth, free_ref.keep_of(0.05), 1, 0.5)
    assert np.array_equal(want["kept"], stays)
    sptr = m.stamps.data_ptr()
    assert m.remove_seen_through(torch.from_numpy(depth), K, torch.from_numpy(_pose()), 0.5) == (n // 2, n // 2)
    assert m.stamps.data_ptr() != sptr and m._free["stamps"].data_ptr() == sptr
    assert np.array_equal(m.stamps[:n // 2].cpu().numpy(), stamps[want["ids"]])
    # the stamps observe() then writes are the mirror's on the rows that are left
    left = means[want["ids"]]
    seen = ref.observed(left, ref.w2c_of(c2w), intr, depth, ref.keep_of(0.05), 1, 4.0, 0.5, 10.0)
    assert seen.any()
    m.frame_index = 2000
    m.observe(torch.from_numpy(depth), K, torch.from_numpy(_pose()), 0.5, 10.0)
    assert m.frame_index == 2001
    assert np.array_equal(m.stamps[:n // 2].cpu().numpy(), ref.stamp(stamps[want["ids"]], seen, 2001))
