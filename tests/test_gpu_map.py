"""GPU: gsl_map_select / gsl_map_append (csrc/map.hip) against the numpy mirror tests/map_ref.py on given arrays.

Shapes (W x H): 1x1; 13x7 less than a wave; 64x1 exactly one wave; 65x3; 256x1 exactly one workgroup; 257x2 the workgroup
seam; 160x120 75 workgroup counts; 640x480 1200 counts, more than the scan workgroup has threads (a thread then owns a
chunk of five).  Patterns: random (about 30 % selected, invalid depths strewn in), none, all, only the last pixel, a
checkerboard, and the "no render yet" form.

Asserted: the two counters and the selected pixel indices (decoded from the ballots the first pass leaves in the
workspace) are exactly the mirror's -- the rule has no rounding freedom on given float32 inputs; every mean component j
is within 8 * 2^-24 * (sum_k |R_jk| |p_k| + |t_j|) of the float64 mirror (two divisions, three multiplications and the
three-term sum, each rounded once, and the float32 chain has no fused operation); colours within one float32 ulp; live
rows, rows past the appended ones and a guard region behind the capacity untouched; two runs bit-identical."""
import numpy as np
import pytest
import torch

from gsplatloc_amd import _lib
from gsplatloc_amd.mapping import GaussianMap, MapConfig
from tests import map_ref
from tests.pose_ref import axis_angle

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
SHAPES = [(1, 1), (13, 7), (64, 1), (65, 3), (256, 1), (257, 2), (160, 120), (640, 480)]
PATTERNS = ["random", "none", "all", "last", "checkerboard", "no_render"]
ALPHA_MIN, KEEP = 0.5, map_ref.keep_of(0.05)
SENTINEL, GUARD = -7.25, 64


def _pose():
    c2w = np.eye(4)
    c2w[:3, :3] = axis_angle((0.4, -0.7, 0.6), 37.0).numpy()
    c2w[:3, 3] = [1.3, -0.8, 2.1]
    return c2w.astype(F32)


def _intr(W, H):
    return (95.3, 88.1, W / 2 - 0.3, H / 2 + 0.2)  # fx != fy, the principal point off the centre


def _inputs(W, H, pattern, seed=0):
    """(d_o, d_r, a, rgb) float32 arrays that realise the pattern under the rule."""
    rng = np.random.default_rng(1000 * W + H + seed)
    d_r = rng.uniform(1.0, 5.0, (H, W)).astype(F32)
    rgb = rng.uniform(0.0, 255.0, (H, W, 3)).astype(F32)
    v, u = np.mgrid[0:H, 0:W]
    d_o, a = d_r.copy(), np.full((H, W), 0.9, F32)  # covered, depths agree: nothing is new
    if pattern in ("random", "no_render"):
        a = (0.5 + 0.5 * rng.random((H, W))).astype(F32)
        low = rng.random((H, W)) < 0.15
        a[low] = (0.5 * rng.random((H, W))).astype(F32)[low]
        d_o = (d_r * rng.uniform(0.9, 1.1, (H, W))).astype(F32)
        bad = rng.random((H, W)) < 0.06
        d_o[bad] = rng.choice(np.array([0.0, -1.5, np.nan, np.inf, -np.inf], F32), int(bad.sum()))
    elif pattern == "all":
        a[:] = 0.1
    elif pattern == "last":
        a[-1, -1] = 0.0
    elif pattern == "checkerboard":
        a[(u + v) % 2 == 0] = 0.1
    if pattern == "no_render":
        return d_o, None, None, rgb
    return d_o, d_r, a, rgb


def _run(W, H, d_o, d_r, a, rgb, n_live, capacity):
    """The two entry points on buffers of capacity + GUARD rows filled with a sentinel (live rows: their index);
    returns (n_new, selected indices from the ballots, means, colors) on the host."""
    lib, ptr = _lib.load_library(), _lib.ptr
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)  # noqa: E731
    d_o_t, d_r_t, a_t, rgb_t, c2w = t(d_o), t(d_r), t(a), t(rgb), t(_pose())
    means = torch.full((capacity + GUARD, 3), SENTINEL, device=DEV)
    colors = torch.full((capacity + GUARD, 3), SENTINEL, device=DEV)
    live = torch.arange(n_live * 3, dtype=torch.float32, device=DEV).reshape(n_live, 3)
    means[:n_live], colors[:n_live] = live, -live
    n_new = torch.full((2,), -5, dtype=torch.int32, device=DEV)
    ws_bytes = lib.gsl_map_ws_bytes(W, H)
    ws = torch.full((ws_bytes + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    st = _lib.current_stream()
    _lib.check(lib.gsl_map_select(ptr(d_r_t), ptr(a_t), ptr(d_o_t), W, H, ALPHA_MIN, float(KEEP), ptr(n_new), ptr(ws),
                                  ws_bytes, st), "gsl_map_select")
    first = n_new.tolist()
    _lib.check(lib.gsl_map_append(ptr(d_o_t), ptr(rgb_t), W, H, *_intr(W, H), ptr(c2w), ptr(means), ptr(colors), n_live,
                                  capacity, ptr(n_new), ptr(ws), ws_bytes, st), "gsl_map_append")
    torch.cuda.synchronize()
    assert bool((ws[ws_bytes:] == 0xAB).all())  # nothing behind the size the library asked for
    nb = (W * H + 255) // 256
    words = ws[:nb * 32].cpu().numpy().view(np.uint64)
    bits = ((words[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool).reshape(-1)
    assert not bits[W * H:].any()  # lanes past the image select nothing
    return first, tuple(n_new.tolist()), np.flatnonzero(bits[:W * H]), means.cpu().numpy(), colors.cpu().numpy()


def _check(W, H, pattern, n_live, capacity):
    d_o, d_r, a, rgb = _inputs(W, H, pattern)
    ref = map_ref.insert(d_o, rgb, _intr(W, H), _pose(), n_live, capacity, d_r, a, ALPHA_MIN, KEEP)
    first, n_new, idx, means, colors = _run(W, H, d_o, d_r, a, rgb, n_live, capacity)
    sel, app = ref["n_new"]
    assert first == [sel, 0]  # after the first pass: the selected count, nothing appended yet
    assert n_new == (sel, app), (n_new, ref["n_new"])
    assert np.array_equal(idx, ref["idx"])
    # rows below n_live and from n_live + appended on, the guard region included, are as they were
    live = np.arange(n_live * 3, dtype=F32).reshape(n_live, 3)
    assert np.array_equal(means[:n_live], live) and np.array_equal(colors[:n_live], -live)
    assert (means[n_live + app:] == SENTINEL).all() and (colors[n_live + app:] == SENTINEL).all()
    got_m, got_c = means[n_live:n_live + app].astype(np.float64), colors[n_live:n_live + app]
    err = np.abs(got_m - ref["means"])
    assert (err <= ref["bound"]).all(), (float((err / ref["bound"]).max()) if app else 0.0)
    ulp = np.spacing(ref["colors"].astype(F32)).astype(np.float64)
    assert (np.abs(got_c.astype(np.float64) - ref["colors"]) <= ulp).all()
    return sel, app, (d_o, d_r, a, rgb), (n_new, idx, means, colors)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_select_and_append_against_the_mirror(shape, pattern):
    W, H = shape
    n_live = 5
    sel, app, inputs, got = _check(W, H, pattern, n_live, n_live + W * H + 3)
    assert app == sel
    want = {"none": 0, "all": W * H, "last": 1, "checkerboard": (W * H + 1) // 2}
    if pattern in want:
        assert sel == want[pattern]
    elif W * H >= 160 * 120:
        frac = sel / (W * H)
        assert (0.25 < frac < 0.45) if pattern == "random" else (0.9 < frac < 0.97), frac
    # a second run: the same bits everywhere (the order is deterministic)
    again = _run(W, H, *inputs, n_live, n_live + W * H + 3)[1:]
    assert again[0] == got[0] and np.array_equal(again[1], got[1])
    assert np.array_equal(again[2].view(np.uint32), got[2].view(np.uint32))
    assert np.array_equal(again[3].view(np.uint32), got[3].view(np.uint32))


def test_rows_beyond_the_capacity_are_dropped():
    """20 x 10 checkerboard: 100 selected, room for 10.  Exactly the first ten (raster order) are appended; the live rows,
    the rows behind them up to the capacity -- none here -- and the guard region behind the capacity are untouched
    (_check asserts all three)."""
    sel, app, _, _ = _check(20, 10, "checkerboard", 7, 17)
    assert (sel, app) == (100, 10)
    # a full map takes nothing, a roomy one everything
    assert _check(20, 10, "checkerboard", 17, 17)[:2] == (100, 0)
    assert _check(20, 10, "checkerboard", 0, 100)[:2] == (100, 100)


def test_gaussian_map_wraps_the_two_entry_points():
    """GaussianMap.insert_frame: the first frame (no render), then a frame with a render, then the capacity."""
    W, H = 65, 3
    m = GaussianMap(W, H, MapConfig(capacity=W * H + 40), DEV)
    assert m.capacity == W * H + 40 and m.n_live == 0 and m.points.shape == (0, 3)
    assert GaussianMap(W, H, MapConfig(), DEV).capacity == 4 * W * H
    K = torch.tensor([[95.3, 0.0, W / 2 - 0.3], [0.0, 88.1, H / 2 + 0.2], [0.0, 0.0, 1.0]])
    d_o, _, _, rgb = _inputs(W, H, "all")
    ref0 = map_ref.insert(d_o, rgb, _intr(W, H), _pose(), 0, m.capacity)
    assert m.insert_frame(d_o, rgb, K, _pose()) == (W * H, W * H) == ref0["n_new"] and not m.full
    assert m.n_live == W * H and m.points.shape == (W * H, 3) and m.point_colors.shape == (W * H, 3)
    assert m.points.data_ptr() == m.means.data_ptr()  # a view of the live prefix
    assert (np.abs(m.points.cpu().numpy() - ref0["means"]) <= ref0["bound"]).all()
    d_o, d_r, a, rgb = _inputs(W, H, "checkerboard")
    ref1 = map_ref.insert(d_o, rgb, _intr(W, H), _pose(), W * H, m.capacity, d_r, a, m.alpha_min, F32(m.keep))
    assert ref1["n_new"] == (98, 40)
    before = m.points.clone()
    assert m.insert_frame(d_o, rgb, K, _pose(), render=d_r, alphas=a) == (98, 40) and m.full
    assert m.n_live == m.capacity and torch.equal(m.points[:W * H], before)
    assert (np.abs(m.points[W * H:].cpu().numpy() - ref1["means"]) <= ref1["bound"]).all()
    assert m.insert_frame(d_o, rgb, K, _pose(), render=d_r, alphas=a) == (98, 0)
    with pytest.raises(ValueError, match="together"):
        m.insert_frame(d_o, rgb, K, _pose(), render=d_r)
    m.clear()
    assert m.n_live == 0 and not m.full
