"""GPU: gsl_map_free_select (csrc/map_free.hip) followed by gsl_map_view_gather against the numpy mirror
tests/map_free_ref.py on given arrays, and GaussianMap.remove_seen_through.

Row counts: 1; 63 / 64 / 65 around one wave; 255 / 256 / 257 around one workgroup; 1000 (four workgroups, the last one
partial); 4099 (17 workgroup counts, three rows in the last).  Windows 0, 1, 2 and 3.  Patterns: every row removed (no
survivor), none removed, every other row stays, only lane 0 / only lane 63 of every wave stays, only the last row stays
-- a 160x120 image under a general pose, the rows that go at 1 .. 2 m in front of a surface at 3 .. 3.1 m, those that
stay behind it -- and a random cloud on a 64x48 image under the pose and intrinsics of tests/test_gpu_map_view.py whose
float32 arithmetic is exact (a quarter turn and a dyadic translation, power-of-two intrinsics) with keep = 0.9375, so
that the hand-made rows (below) sit on their thresholds on the device as well; the depth image varies with both pixel
coordinates and has patches of 0, NaN, +inf, -1 and -inf.

Every case asserts: the counters after each of the two calls; the ballot bits; out_ids strictly ascending and the
mirror's; means / colours bit copies of the rows at those ids; the sentinel rows past the count, a guard region behind
the outputs and the bytes behind the workspace untouched; means, colors and depth unchanged.  The rule has no rounding
freedom on given float32 inputs: everything is compared for equality.

No time is asserted.  Measured on the MI355X (one kernel trace of its own, 640x480, 313 k .. 375 k rows, window 1):
k_map_free_select 6.7 .. 8.2 us, mean 7.4; k_map_view_gather after it 4.5 .. 6.8 us (NOTES.md, "Free space")."""
import numpy as np
import pytest
import torch

from gsplatloc_amd import _lib
from gsplatloc_amd.mapping import GaussianMap, MapConfig
from tests import map_free_ref as ref
from tests import map_view_ref as view_ref
from tests.test_gpu_map_view import EH, EINTR, EW, GUARD_ROWS, H, INTR, SENTINEL, W, _exact_pose, _pose, _world

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
ROWS = [1, 63, 64, 65, 255, 256, 257, 1000, 4099]
PATTERNS = ["all_removed", "none_removed", "every_other", "lane0", "lane63", "last", "random"]
WINDOWS = [0, 1, 2, 3]
NEAR = 0.5
KEEP, EKEEP = ref.keep_of(0.05), F32(0.9375)  # the exact case: d * keep is exact for the dyadic depths below
D_STEP = float(np.nextafter(F32(2.0), F32(9)))  # 2 + 2^-22: times 0.9375 it rounds to 1.875 + 2^-22


def _exact_depth():
    """[EH,EW]: 2 + (u + 2 v) / 64 (2 .. 4.5 m, dyadic, another value on every neighbour), a 7x7 patch at exactly 2 m and
    one a float32 step above, one close pixel, and patches without depth."""
    v, u = np.meshgrid(np.arange(EH), np.arange(EW), indexing="ij")
    d = (2.0 + (u + 2.0 * v) / 64.0).astype(F32)
    d[4:11, 4:11] = 2.0
    d[4:11, 16:23] = D_STEP
    d[30, 11] = 0.75
    d[30:34, 40:46], d[20:23, 50:54] = 0.0, np.nan
    d[5, 40], d[40, 10], d[44, 60] = np.inf, -1.0, -np.inf
    return d


def _specials():
    """Hand-made rows in the camera frame of the exact pose (u = 64 x / z + 32, v = 64 y / z + 24), and what the rule says
    of them with window 0: (rows [13,3], stays [13])."""
    at = lambda u, v, z: [(u - 32.0) / 64.0 * z, (v - 24.0) / 64.0 * z, z]  # noqa: E731
    rows = [at(7, 7, 1.875),  # z == d * keep in the 2 m patch: stays
            at(19, 7, 1.875),  # the patch a step above: d * keep is one step above z, goes
            at(-0.5, 20, 1.0),  # rounds to -0: column 0, goes
            at(-0.5 - 2.0 ** -17, 20, 1.0),  # rounds to -1: untested
            at(10.5, 30, 1.0),  # column 10 (half to even; column 11 is the close pixel), goes
            at(11.5, 30, 1.0),  # column 12, goes
            at(11, 30, 1.0),  # the close pixel itself: blocked
            at(32, 24, NEAR),  # on the near plane: untested
            at(EW - 1 + 0.5, 24, 1.0),  # rounds to EW: untested
            [np.nan, 0.0, 1.0], [0.0, 0.0, np.nan], [np.inf, 0.0, 1.0], [0.0, 0.0, -np.inf]]
    return np.array(rows), np.array([True, False, False, True, False, False, True, True, True, True, True, True, True])


def _random_case(n):
    """A cloud that straddles the frustum of the exact pose with the hand-made rows (fewer when n < 13) at ``where``.
    Returns (means in the world, where)."""
    rng = np.random.default_rng(100 * n + 1)
    z = rng.uniform(0.3, 4.0, n)
    u, v = rng.uniform(-6.0, EW + 5.0, n), rng.uniform(-6.0, EH + 5.0, n)
    p = np.stack([(u - 32.0) / 64.0 * z, (v - 24.0) / 64.0 * z, z], axis=-1)
    rows, _ = _specials()
    where = rng.permutation(n)[:min(n, len(rows))]
    p[where] = rows[:len(where)]
    with np.errstate(invalid="ignore"):
        return _world(p, _exact_pose()), where


def _case(n, pattern):
    """(means [n,3] float32 in the world, c2w, intrinsics, depth [h,w] float32, keep, the rows the pattern means to stay
    or None)."""
    rng = np.random.default_rng(100 * n + len(pattern))
    i = np.arange(n)
    if pattern == "random":
        return _random_case(n)[0], _exact_pose(), EINTR, _exact_depth(), EKEEP, None
    stays = {"all_removed": i < 0, "none_removed": i >= 0, "every_other": i % 2 == 0, "lane0": i % 64 == 0,
             "lane63": i % 64 == 63, "last": i == n - 1}[pattern]
    u, v = rng.uniform(5.0, W - 6.0, n), rng.uniform(5.0, H - 6.0, n)  # well inside: the window never leaves the image
    z = np.where(stays, rng.uniform(3.2, 3.5, n), rng.uniform(1.0, 2.0, n))  # behind / in front of 3 .. 3.1 m
    p = np.stack([(u - INTR[2]) / INTR[0] * z, (v - INTR[3]) / INTR[1] * z, z], axis=-1)
    depth = rng.uniform(3.0, 3.1, (H, W)).astype(F32)
    return _world(p, _pose()), _pose(), INTR, depth, KEEP, stays


def _run(means, colors, w2c, intr, depth, keep, window):
    """The entry point and the gather on outputs of n + 3 + GUARD_ROWS sentinel rows; the counters after each call and
    everything that was written, on the host."""
    lib, ptr, st = _lib.load_library(), _lib.ptr, _lib.current_stream()
    n, (h, w) = means.shape[0], depth.shape
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    m_t, c_t, w_t, d_t = t(means), t(colors), t(w2c), t(depth)
    rows = n + 3 + GUARD_ROWS
    out_m = torch.full((rows, 3), SENTINEL, device=DEV)
    out_c = torch.full((rows, 3), SENTINEL, device=DEV)
    out_i = torch.full((rows,), -77, dtype=torch.int32, device=DEV)
    counters = torch.full((3,), -5, dtype=torch.int32, device=DEV)
    ws_bytes = lib.gsl_map_view_ws_bytes(n)
    ws = torch.full((ws_bytes + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    _lib.check(lib.gsl_map_free_select(ptr(m_t), n, ptr(w_t), *intr, ptr(d_t), w, h, float(keep), window, NEAR,
                                       ptr(counters), ptr(ws), ws_bytes, st), "gsl_map_free_select")
    first = counters.tolist()
    _lib.check(lib.gsl_map_view_gather(ptr(m_t), ptr(c_t), n, ptr(out_m), ptr(out_c), ptr(out_i), n + 3, ptr(counters),
                                       ptr(ws), ws_bytes, st), "gsl_map_view_gather")
    torch.cuda.synchronize()
    assert bool((ws[ws_bytes:] == 0xAB).all())  # nothing behind the size the library asked for
    # the inputs are only read (bit comparison: the cloud holds NaNs)
    for dev, host in ((m_t, means), (c_t, colors), (d_t, depth)):
        assert np.array_equal(dev.cpu().numpy().view(np.uint32), np.ascontiguousarray(host).view(np.uint32))
    nb = (n + 255) // 256
    words = ws[:nb * 32].cpu().numpy().view(np.uint64)
    bits = ((words[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool).reshape(-1)
    assert not bits[n:].any()  # lanes past the last row keep nothing
    return dict(first=first, counters=counters.tolist(), bits=bits[:n], ids=out_i.cpu().numpy(),
                means=out_m.cpu().numpy(), colors=out_c.cpu().numpy())


def _check_outputs(got, want_ids, means, colors):
    k = len(want_ids)
    assert np.array_equal(got["ids"][:k], want_ids) and (np.diff(got["ids"][:k]) > 0).all()
    assert np.array_equal(got["means"][:k].view(np.uint32), means[want_ids].view(np.uint32))
    assert np.array_equal(got["colors"][:k].view(np.uint32), colors[want_ids].view(np.uint32))
    assert (got["ids"][k:] == -77).all() and (got["means"][k:] == SENTINEL).all() and (got["colors"][k:] == SENTINEL).all()
    assert got["ids"].shape[0] == means.shape[0] + 3 + GUARD_ROWS


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", ROWS)
def test_select_and_gather_against_the_mirror(n, pattern, window):
    means, c2w, intr, depth, keep, intended = _case(n, pattern)
    colors = np.random.default_rng(n).uniform(0.0, 1.0, (n, 3)).astype(F32)
    w2c = ref.w2c_of(c2w)
    want = ref.select(means, w2c, intr, depth, keep, window, NEAR)
    if intended is not None:
        assert np.array_equal(want["kept"], intended) and want["tested"].all()  # the case is what it says
    elif n == 4099:
        gone = (~want["kept"]).sum() / want["tested"].sum()
        assert 0.1 <= gone <= 0.8 and 0.3 < want["tested"].mean() < 0.95, (gone, want["tested"].mean())
    got = _run(means, colors, w2c, intr, depth, keep, window)
    stay = want["counters"][0]
    assert got["first"] == [stay, 0, 0]  # after the first call: the rows that stay, nothing gathered
    assert tuple(got["counters"]) == want["counters"] == (stay, 0, stay)
    assert np.array_equal(got["bits"], want["kept"])
    _check_outputs(got, want["ids"], means, colors)


@pytest.mark.parametrize("window", WINDOWS)
def test_the_hand_made_rows_are_where_the_mirror_puts_them(window):
    """The random case at 4099 rows holds the hand-made rows: on the threshold stays, a step below goes, -0.5 is column
    0, halves go to the even column, the near plane, the far border and NaN / inf rows are untested -- on the device as
    in the mirror (asserted above), and here that the verdict is the intended one.  The windows above 0 reach the
    close pixel and the border of the 2 m patch's neighbour: rows 4 and 5 then stay, all else is as with window 0."""
    means, where = _random_case(4099)
    _, stays = _specials()
    stays = stays.copy()
    if window >= 1:
        stays[[4, 5]] = True  # column 11, the close pixel, is in their window now
    w2c = ref.w2c_of(_exact_pose())
    kept, tested = ref.rule(means, w2c, EINTR, _exact_depth(), EKEEP, window, NEAR)
    assert kept[where].tolist() == stays.tolist()
    assert tested[where].tolist() == [True, True, True, False, True, True, True] + [False] * 6
    got = _run(means, np.zeros_like(means), w2c, EINTR, _exact_depth(), EKEEP, window)
    assert got["bits"][where].tolist() == stays.tolist()


def _map_with(means, colors, cap, **cfg):
    m = GaussianMap(W, H, MapConfig(capacity=cap, **cfg), DEV)
    n = means.shape[0]
    m.means[:n], m.colors[:n], m.n_live = torch.from_numpy(means).to(DEV), torch.from_numpy(colors).to(DEV), n
    return m


def test_gaussian_map_removes_what_the_mirror_removes():
    n, cap = 1000, 1500
    K = torch.tensor([[INTR[0], 0.0, INTR[2]], [0.0, INTR[1], INTR[3]], [0.0, 0.0, 1.0]])
    intr = tuple(float(F32(a)) for a in INTR)
    colors = np.random.default_rng(5).uniform(0.0, 1.0, (n, 3)).astype(F32)
    pose = torch.from_numpy(_pose())
    means, c2w, _, depth, _, _ = _case(n, "none_removed")
    # a frame that observes 10 m everywhere sees through every row
    m = _map_with(means, colors, cap, free_rho=0.05)
    assert m.remove_seen_through(torch.full((H, W), 10.0), K, pose, NEAR) == (n, 0) and m.n_live == 0
    assert m.survivors.numel() == 0 and m.points.shape == (0, 3)
    # nothing is seen through: the same buffers, the same rows
    m = _map_with(means, colors, cap, free_rho=0.05)
    ptr, m._view_rows = m.means.data_ptr(), n
    assert m.remove_seen_through(torch.from_numpy(depth), K, pose, NEAR) == (0, n)
    assert m.means.data_ptr() == ptr and m.n_live == n == m._view_rows
    assert np.array_equal(m.survivors.cpu().numpy(), np.arange(n, dtype=np.int32))
    # every other row goes
    means, c2w, _, depth, _, stays = _case(n, "every_other")
    for window in (0, 1, 3):
        m = _map_with(means, colors, cap, free_rho=0.05, free_window_px=window)
        want = ref.select(means, ref.w2c_of(c2w), intr, depth, ref.keep_of(0.05), window, NEAR)
        assert np.array_equal(want["kept"], stays)
        ptr, cptr = m.means.data_ptr(), m.colors.data_ptr()
        m.select_view(K, pose, 8.0, NEAR, 10.0)
        assert m._view_rows == n and m.view_violations(K, pose, NEAR, 10.0) == 0
        removed, kept = m.remove_seen_through(torch.from_numpy(depth).to(DEV), K, pose.to(DEV), NEAR)
        assert (removed, kept) == (n - want["counters"][0], want["counters"][0]) == (n // 2, n // 2) and m.n_live == kept
        assert m.means.data_ptr() != ptr and m.colors.data_ptr() != cptr and m._free["means"].data_ptr() == ptr
        assert m.means.shape == (cap, 3) and m.survivors.dtype == torch.int32
        assert np.array_equal(m.survivors.cpu().numpy(), want["ids"])
        assert np.array_equal(m.points.cpu().numpy().view(np.uint32), means[want["ids"]].view(np.uint32))
        assert np.array_equal(m.point_colors.cpu().numpy().view(np.uint32), colors[want["ids"]].view(np.uint32))
        # the view ballots describe other rows now
        with pytest.raises(RuntimeError, match="select_view"):
            m.view_violations(K, pose, NEAR, 10.0)
        sel = view_ref.select(means[want["ids"]], view_ref.w2c_of(_pose()), intr, W, H, 8.0, NEAR, 10.0)
        pts, _, ids, k = m.select_view(K, pose, 8.0, NEAR, 10.0)
        assert k == sel["counters"][0] == kept and np.array_equal(ids.cpu().numpy(), sel["ids"])
        assert torch.equal(pts, m.points[ids.long()]) and m.view_violations(K, pose, NEAR, 10.0) == 0
        # a second removal with the same frame: nothing more, nothing swapped
        ptr = m.means.data_ptr()
        assert m.remove_seen_through(torch.from_numpy(depth), K, pose, NEAR) == (0, kept) and m.means.data_ptr() == ptr
