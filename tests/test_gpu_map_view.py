"""GPU: gsl_map_view_select / gsl_map_view_gather (csrc/map_view.hip) against the numpy mirror tests/map_view_ref.py on
given arrays.

Row counts: 1; 63 / 64 / 65 around one wave; 255 / 256 / 257 around one workgroup; 1000 (four workgroups, the last one
partial); 4099 (17 workgroup counts, three rows in the last); 66 000 (258 workgroup counts: the scan's threads own
chunks of two, and those from 129 on own nothing -- also under the check against an earlier selection, the one call that
runs two scans).  Patterns: all rows in view, none (all behind the camera),
every other row, only lane 0 / only lane 63 of every wave, only the last row -- under a general pose -- and a random
cloud that straddles the frustum, with rows exactly on the four borders and the two depth planes and NaN / inf rows
mixed in, under a pose whose float32 arithmetic is exact (a quarter turn and a dyadic translation, power-of-two
intrinsics), so that the border rows sit on the borders on the device as well.

Every case asserts: the three counters are the mirror's; out_ids are the mirror's, strictly ascending; out_means /
out_colors are bit copies of the map rows at those ids; the rows past the count of sentinel-filled outputs, a guard
region behind them and the bytes behind the workspace are untouched; a second gather with a capacity below the count
writes exactly that many rows and reports it.  The rule has no rounding freedom on given float32 inputs: everything is
compared for equality."""
import numpy as np
import pytest
import torch

from gsplatloc_amd import _lib
from gsplatloc_amd.mapping import GaussianMap, MapConfig
from tests import map_view_ref as ref
from tests.pose_ref import axis_angle

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
ROWS = [1, 63, 64, 65, 255, 256, 257, 1000, 4099, 66000]
PATTERNS = ["all", "none", "every_other", "lane0", "lane63", "last", "random"]
SENTINEL, GUARD_ROWS = -7.25, 64
W, H, INTR = 160, 120, (95.3, 88.1, 160 / 2 - 0.3, 120 / 2 + 0.2)  # fx != fy, the principal point off the centre
EW, EH, EINTR = 64, 48, (64.0, 64.0, 32.0, 24.0)  # the exact case: u = 64 x + 32, v = 64 y + 24 at z = 1
NEAR, FAR, GUARD = 0.5, 4.0, 8.0


def _pose(deg=37.0, t=(1.3, -0.8, 2.1)):
    c2w = np.eye(4)
    c2w[:3, :3] = axis_angle((0.4, -0.7, 0.6), deg).numpy()
    c2w[:3, 3] = t
    return c2w


def _exact_pose():
    """A quarter turn about z and a dyadic translation: every product and sum of the rule is exact for dyadic rows."""
    c2w = np.eye(4)
    c2w[:3, :3] = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
    c2w[:3, 3] = [0.5, -0.25, 2.0]
    return c2w


def _world(p_cam, c2w):
    return (p_cam @ c2w[:3, :3].T + c2w[:3, 3]).astype(F32)


def _random_case(n):
    """A cloud that straddles the frustum of the exact pose; 16 of its rows (fewer when n < 16), at ``where``, are: on the
    four borders and on a corner (5 rows, in view); on the near and on the far plane, 2^-14 px beyond the left and beyond
    the lower border (4 rows, out); NaN / inf coordinates (7 rows, out).  Returns (means in the world, where)."""
    rng = np.random.default_rng(100 * n)
    z = rng.uniform(0.3, 5.0, n)
    p = np.stack([rng.uniform(-1.2, 1.2, n) * z, rng.uniform(-1.0, 1.0, n) * z, z], axis=-1)
    x = lambda u: (u - 32.0) / 64.0  # noqa: E731
    y = lambda v: (v - 24.0) / 64.0  # noqa: E731
    special = [[x(-GUARD), 0.0, 1.0], [x(EW - 1 + GUARD), 0.0, 1.0], [0.0, y(-GUARD), 1.0],
               [0.0, y(EH - 1 + GUARD), 1.0], [x(-GUARD), y(EH - 1 + GUARD), 1.0], [0.0, 0.0, NEAR], [0.0, 0.0, FAR],
               [x(-GUARD) - 2.0 ** -20, 0.0, 1.0], [0.0, y(EH - 1 + GUARD) + 2.0 ** -20, 1.0],
               [np.nan, 0.0, 1.0], [0.0, 0.0, np.nan], [np.inf, 0.0, 1.0], [0.0, -np.inf, 1.0], [0.0, 0.0, np.inf],
               [0.0, 0.0, -np.inf], [np.nan, np.nan, np.nan]]
    where = rng.permutation(n)[:min(n, len(special))]
    p[where] = np.array(special)[:len(where)]
    with np.errstate(invalid="ignore"):
        return _world(p, _exact_pose()), where


def _case(n, pattern):
    """(means [n,3] float32 in the world, c2w, intrinsics, width, height, the mask the pattern intends or None)."""
    rng = np.random.default_rng(100 * n + len(pattern))
    i = np.arange(n)
    if pattern == "random":
        return _random_case(n)[0], _exact_pose(), EINTR, EW, EH, None
    c2w, intr, w, h = _pose(), INTR, W, H
    mask = {"all": i >= 0, "none": i < 0, "every_other": i % 2 == 0, "lane0": i % 64 == 0, "lane63": i % 64 == 63,
            "last": i == n - 1}[pattern]
    z = rng.uniform(1.0, 3.5, n)
    u, v = rng.uniform(5.0, w - 6.0, n), rng.uniform(5.0, h - 6.0, n)  # well inside the image: rounding cannot move it out
    p = np.stack([(u - intr[2]) / intr[0] * z, (v - intr[3]) / intr[1] * z, z], axis=-1)
    p[~mask] *= -1.0  # behind the camera
    return _world(p, c2w), c2w, intr, w, h, mask


def _run(means, colors, w2c, intr, w, h, guard, capacity, prev_ws=None, gather=True):
    """The two entry points on outputs of capacity + GUARD_ROWS sentinel rows; (counters after select, counters after
    gather, ids, means, colors, workspace tensor) with the arrays on the host."""
    lib, ptr, st = _lib.load_library(), _lib.ptr, _lib.current_stream()
    n = means.shape[0]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    m_t, c_t, w_t = t(means), t(colors), t(w2c)
    rows = capacity + GUARD_ROWS
    out_m = torch.full((rows, 3), SENTINEL, device=DEV)
    out_c = torch.full((rows, 3), SENTINEL, device=DEV)
    out_i = torch.full((rows,), -77, dtype=torch.int32, device=DEV)
    counters = torch.full((3,), -5, dtype=torch.int32, device=DEV)
    ws_bytes = lib.gsl_map_view_ws_bytes(n)
    ws = torch.full((ws_bytes + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    _lib.check(lib.gsl_map_view_select(ptr(m_t), n, ptr(w_t), *intr, w, h, guard, NEAR, FAR, ptr(prev_ws), ptr(counters),
                                       ptr(ws), ws_bytes, st), "gsl_map_view_select")
    first = counters.tolist()
    if gather:
        _lib.check(lib.gsl_map_view_gather(ptr(m_t), ptr(c_t), n, ptr(out_m), ptr(out_c), ptr(out_i), capacity,
                                           ptr(counters), ptr(ws), ws_bytes, st), "gsl_map_view_gather")
    torch.cuda.synchronize()
    assert bool((ws[ws_bytes:] == 0xAB).all())  # nothing behind the size the library asked for
    nb = (n + 255) // 256
    words = ws[:nb * 32].cpu().numpy().view(np.uint64)
    bits = ((words[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool).reshape(-1)
    assert not bits[n:].any()  # lanes past the last row select nothing
    return dict(first=first, counters=counters.tolist(), bits=bits[:n], ids=out_i.cpu().numpy(),
                means=out_m.cpu().numpy(), colors=out_c.cpu().numpy(), ws=ws)


def _check_outputs(got, want_ids, means, colors, capacity):
    k = len(want_ids)
    assert np.array_equal(got["ids"][:k], want_ids) and (np.diff(got["ids"][:k]) > 0).all()
    assert np.array_equal(got["means"][:k].view(np.uint32), means[want_ids].view(np.uint32))
    assert np.array_equal(got["colors"][:k].view(np.uint32), colors[want_ids].view(np.uint32))
    assert (got["ids"][k:] == -77).all() and (got["means"][k:] == SENTINEL).all() and (got["colors"][k:] == SENTINEL).all()
    assert got["ids"].shape[0] == capacity + GUARD_ROWS


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", ROWS)
def test_select_and_gather_against_the_mirror(n, pattern):
    means, c2w, intr, w, h, intended = _case(n, pattern)
    colors = np.random.default_rng(n).uniform(0.0, 1.0, (n, 3)).astype(F32)
    w2c = ref.w2c_of(c2w)
    want = ref.select(means, w2c, intr, w, h, GUARD, NEAR, FAR, out_capacity=n + 3)
    if intended is not None:
        assert np.array_equal(want["mask"], intended)  # the case is what it says
    elif n >= 1000:
        assert 0.1 < want["mask"].mean() < 0.8, want["mask"].mean()  # the cloud does straddle the frustum
    got = _run(means, colors, w2c, intr, w, h, GUARD, n + 3)
    sel = want["counters"][0]
    assert got["first"] == [sel, 0, 0]  # after the first pass: the count, no earlier selection, nothing gathered
    assert tuple(got["counters"]) == want["counters"] == (sel, 0, sel)
    assert np.array_equal(got["bits"], want["mask"])
    _check_outputs(got, want["ids"], means, colors, n + 3)
    # a capacity below the count: exactly that many rows, in order, and the counter says so
    cap = sel // 2
    if sel > 0:
        clamped = _run(means, colors, w2c, intr, w, h, GUARD, cap)
        assert tuple(clamped["counters"]) == ref.select(means, w2c, intr, w, h, GUARD, NEAR, FAR, cap)["counters"]
        assert clamped["counters"] == [sel, 0, cap]
        _check_outputs(clamped, want["ids"][:cap], means, colors, cap)


def test_the_exact_border_rows_are_where_the_mirror_puts_them():
    """The random case at 4099 rows holds the border rows: on the four borders in, on either depth plane out, one step
    of u / v beyond a border out, NaN / inf rows out -- on the device as in the mirror (asserted above), and here that
    the mirror's verdict on them is the intended one."""
    means, where = _random_case(4099)
    w2c = ref.w2c_of(_exact_pose())
    assert ref.in_view(means, w2c, EINTR, EW, EH, GUARD, NEAR, FAR)[where].tolist() == [True] * 5 + [False] * 11
    got = _run(means, np.zeros_like(means), w2c, EINTR, EW, EH, GUARD, 4099)
    assert got["bits"][where].tolist() == [True] * 5 + [False] * 11


def _violation_case(n):
    """(means [n,3] in the world that straddle the frustum of pose A, colors, w2c of pose A, w2c of a pose B nearby)."""
    rng = np.random.default_rng(7)
    z = rng.uniform(0.8, 3.8, n)
    p = np.stack([rng.uniform(-1.3, 1.3, n) * z, rng.uniform(-1.1, 1.1, n) * z, z], axis=-1)  # straddles the frustum
    pose_a, pose_b = _pose(37.0), _pose(39.5, (1.32, -0.79, 2.08))
    means, colors = _world(p, pose_a), rng.uniform(0.0, 1.0, (n, 3)).astype(F32)
    return means, colors, ref.w2c_of(pose_a), ref.w2c_of(pose_b)


def test_violations_against_an_earlier_selection():
    _violations_against_an_earlier_selection(4099)


def test_violations_against_an_earlier_selection_with_two_counts_per_scan_thread():
    _violations_against_an_earlier_selection(66000)


def _violations_against_an_earlier_selection(n):
    means, colors, w2c_a, w2c_b = _violation_case(n)
    a = _run(means, colors, w2c_a, INTR, W, H, GUARD, n)
    mask_a = ref.in_view(means, w2c_a, INTR, W, H, GUARD, NEAR, FAR)
    assert np.array_equal(a["bits"], mask_a) and 0.2 < mask_a.mean() < 0.8
    before = a["ws"].clone()
    # pose B with the reach, against A's ballots
    want = ref.select(means, w2c_b, INTR, W, H, 4.0, NEAR, FAR, prev=mask_a)
    b = _run(means, colors, w2c_b, INTR, W, H, 4.0, n, prev_ws=a["ws"], gather=False)
    assert want["counters"][1] > 0 and b["counters"] == [want["counters"][0], want["counters"][1], 0]
    assert np.array_equal(b["bits"], want["mask"]) and torch.equal(a["ws"], before)  # prev_ws is only read
    # the same pose with a smaller guard: everything it sees was selected
    same = _run(means, colors, w2c_a, INTR, W, H, 4.0, n, prev_ws=a["ws"], gather=False)
    assert same["counters"][1] == 0 and 0 < same["counters"][0] <= a["counters"][0]
    # ... and a wider one: the band between the two
    wider = _run(means, colors, w2c_a, INTR, W, H, 20.0, n, prev_ws=a["ws"], gather=False)
    assert wider["counters"][1] == wider["counters"][0] - a["counters"][0] > 0
    assert wider["counters"][1] == ref.violations(means, w2c_a, INTR, W, H, 20.0, NEAR, FAR, mask_a)


def test_gaussian_map_wraps_the_two_entry_points():
    n, cap = 1000, 1500
    rng = np.random.default_rng(3)
    z = rng.uniform(0.8, 3.8, n)
    p = np.stack([rng.uniform(-1.3, 1.3, n) * z, rng.uniform(-1.1, 1.1, n) * z, z], axis=-1)
    pose_a, pose_b = _pose(37.0), _pose(40.0)
    means, colors = _world(p, pose_a), rng.uniform(0.0, 1.0, (n, 3)).astype(F32)
    m = GaussianMap(W, H, MapConfig(capacity=cap, view_guard_px=GUARD, view_reach_px=4.0), DEV)
    K = torch.tensor([[INTR[0], 0.0, INTR[2]], [0.0, INTR[1], INTR[3]], [0.0, 0.0, 1.0]])
    with pytest.raises(RuntimeError, match="select_view"):
        m.view_violations(K, torch.from_numpy(pose_a), NEAR, FAR)
    assert m.select_view(K, torch.from_numpy(pose_a), GUARD, NEAR, FAR)[3] == 0  # an empty map: nothing, no launch
    m.means[:n], m.colors[:n], m.n_live = torch.from_numpy(means).to(DEV), torch.from_numpy(colors).to(DEV), n
    intr = tuple(float(F32(a)) for a in INTR)
    want = ref.select(means, ref.w2c_of(pose_a), intr, W, H, GUARD, NEAR, FAR)
    pts, col, ids, k = m.select_view(K, torch.from_numpy(pose_a).to(DEV), GUARD, NEAR, FAR)
    assert k == want["counters"][0] and 0 < k < n and pts.shape == col.shape == (k, 3) and ids.dtype == torch.int32
    assert np.array_equal(ids.cpu().numpy(), want["ids"])
    assert torch.equal(pts, m.means[ids.long()]) and torch.equal(col, m.colors[ids.long()])
    assert pts.data_ptr() == m._view["means"].data_ptr() and m._view["means"].shape == (cap, 3)  # a view of the prefix
    assert m.view_violations(K, torch.from_numpy(pose_a), NEAR, FAR) == 0
    v = m.view_violations(K, torch.from_numpy(pose_b), NEAR, FAR)
    assert v == ref.violations(means, ref.w2c_of(pose_b), intr, W, H, 4.0, NEAR, FAR, want["mask"]) > 0
    assert torch.equal(pts, m.means[ids.long()])  # the check gathers nothing
    m.n_live = n - 1
    with pytest.raises(RuntimeError, match="select_view"):  # the ballots describe other rows
        m.view_violations(K, torch.from_numpy(pose_a), NEAR, FAR)
    m.clear()
    assert m.n_live == 0 and m._view_rows == -1
