"""GPU: gsl_map_occl_depth / gsl_map_occl_select (csrc/map_occl.hip), followed by the unchanged gsl_map_view_gather,
against the numpy mirror tests/map_occl_ref.py on given arrays: the z-buffer, the ballots' mask, the ids and all four
counters are compared for equality -- the rule has no rounding freedom on given float32 inputs, and the z-buffer is made
with integer atomics.

Row counts: 1; 63 / 64 / 65 around one wave; 255 / 256 / 257 around one workgroup; 1000; 4099 (17 workgroup counts);
66 000 (258 workgroup counts: two per thread of the scans).  Scenes, in the camera's pixels and back-projected:
  two_walls     a far wall over the whole band and, after it in the map, a front wall over the left half, both as
                lattices in raster order (neighbouring lanes share a cell); from 4099 rows on, with the default cell
                and window, the mirror culls at least a quarter of the rows and keeps at least a quarter (asserted);
  equal_depths  the same lattices at one depth: nothing is culled (asserted);
  one_cell_*    every row in one 4-pixel cell, depths ascending / descending / shuffled: the most contention on one
                word and the longest run of equal cells in a wave;
  runs          runs of equal cells of 31, 1, 1, 31, 96 and 200 rows, over and over: they start and end at lanes 0, 31,
                32 and 63 and span a wave and a workgroup boundary (asserted on the mirror's cells);
  sparse        rows 10 pixels apart in a 2600 x 2600 image: with cells up to 4 pixels and a window up to 1 no window
                holds another row, nothing is culled (asserted);
  random        the straddling cloud of tests/test_gpu_map_view.py with rows exactly on the band's borders and the depth
                planes and NaN / inf rows, under the pose whose float32 arithmetic is exact.
Every (rows, scene) pair runs five (cell_px, window) pairs that between them hold every cell size and every window;
test_every_cell_and_window runs all twenty on two scenes."""
import numpy as np
import pytest
import torch

from gsplatloc_amd import _lib
from gsplatloc_amd.mapping import GaussianMap, MapConfig
from tests import map_occl_ref as ref
from tests import test_gpu_map_view as gpu

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
ROWS = gpu.ROWS
SCENES = ["two_walls", "equal_depths", "one_cell_ascending", "one_cell_descending", "one_cell_shuffled", "runs", "sparse",
          "random"]
PAIRS = [(1, 0), (2, 1), (4, 1), (8, 2), (16, 3)]  # (cell_px, window)
W, H, INTR = gpu.W, gpu.H, gpu.INTR
NEAR, FAR, GUARD, RHO = 0.5, 8.0, 8.0, 0.05
SENTINEL, GUARD_ROWS = gpu.SENTINEL, gpu.GUARD_ROWS
RUN_LENGTHS = [31, 1, 1, 31, 96, 200]


def _lattice(m, u0, u1, v0, v1):
    """m points of a regular lattice over [u0, u1] x [v0, v1], in raster order."""
    if m == 0:
        return np.zeros((0, 2))
    cols = max(1, int(np.ceil(np.sqrt(m * (u1 - u0) / (v1 - v0)))))
    lines = -(-m // cols)
    i = np.arange(m)
    return np.stack([u0 + (i % cols + 0.5) * (u1 - u0) / cols, v0 + (i // cols + 0.5) * (v1 - v0) / lines], axis=-1)


def _back(uv, z, intr):
    return np.stack([(uv[:, 0] - intr[2]) / intr[0] * z, (uv[:, 1] - intr[3]) / intr[1] * z, z], axis=-1)


def _case(n, scene):
    """(means [n,3] float32 in the world, c2w, intrinsics, width, height)."""
    rng = np.random.default_rng(1000 * n + len(scene))
    if scene == "random":
        return gpu._random_case(n)[0], gpu._exact_pose(), gpu.EINTR, gpu.EW, gpu.EH
    if scene in ("two_walls", "equal_depths"):
        n_front = n // 3
        far = _lattice(n - n_front, -6.0, W + 5.0, -6.0, H + 5.0)
        front = _lattice(n_front, -6.0, W / 2.0, -6.0, H + 5.0)
        z_far = 3.0 + 0.002 * far[:, 0] if scene == "two_walls" else np.full(len(far), 2.0)
        z_front = np.full(len(front), 1.5 if scene == "two_walls" else 2.0)
        p = np.concatenate([_back(far, z_far, INTR), _back(front, z_front, INTR)])
        return gpu._world(p, gpu._pose()), gpu._pose(), INTR, W, H
    if scene.startswith("one_cell"):
        uv = np.stack([rng.uniform(40.5, 43.5, n), rng.uniform(40.5, 43.5, n)], axis=-1)
        z = 1.0 + 2.0 * np.arange(n) / max(n, 1)
        z = {"ascending": z, "descending": z[::-1].copy(), "shuffled": rng.permutation(z)}[scene.split("_")[-1]]
        return gpu._world(_back(uv, z, INTR), gpu._pose()), gpu._pose(), INTR, W, H
    if scene == "runs":
        _, ch, cw = ref.grid(gpu.EW, gpu.EH, GUARD, 4)
        run = np.repeat(np.arange(n), np.resize(RUN_LENGTHS, n))[:n]  # the run every row belongs to
        cu, cv = (3 * run) % (cw - 2) + 1, (5 * run) % (ch - 2) + 1
        uv = np.stack([4.0 * cu - GUARD + rng.uniform(0.5, 3.5, n), 4.0 * cv - GUARD + rng.uniform(0.5, 3.5, n)], axis=-1)
        return (gpu._world(_back(uv, rng.uniform(1.0, 3.0, n), gpu.EINTR), gpu._exact_pose()), gpu._exact_pose(),
                gpu.EINTR, gpu.EW, gpu.EH)
    assert scene == "sparse"
    side = int(np.ceil(np.sqrt(n)))
    i = np.arange(n)
    uv = np.stack([5.0 + 10.0 * (i % side), 5.0 + 10.0 * (i // side)], axis=-1)
    intr = (1500.0, 1400.0, 1300.0, 1290.0)
    return gpu._world(_back(uv, rng.uniform(1.0, 3.0, n), intr), gpu._pose()), gpu._pose(), intr, 2600, 2600


def _run(means, colors, w2c, intr, w, h, guard, cell, window, rho, capacity, prev_ws=None, gather=True):
    """The two entry points and the gather on sentinel-filled outputs; everything they left, on the host."""
    lib, ptr, st = _lib.load_library(), _lib.ptr, _lib.current_stream()
    n = means.shape[0]
    t = lambda a: torch.from_numpy(np.array(a)).to(DEV)  # noqa: E731  (a copy: the shared cases are read-only)
    m_t, c_t, w_t = t(means), t(colors), t(w2c)
    rows = capacity + GUARD_ROWS
    out_m = torch.full((rows, 3), SENTINEL, device=DEV)
    out_c = torch.full((rows, 3), SENTINEL, device=DEV)
    out_i = torch.full((rows,), -77, dtype=torch.int32, device=DEV)
    counters = torch.full((4,), -5, dtype=torch.int32, device=DEV)
    ws_bytes = lib.gsl_map_occl_ws_bytes(n)
    ws = torch.full((ws_bytes + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    gi, ch, cw = ref.grid(w, h, guard, cell)
    z_bytes = lib.gsl_map_occl_zbuf_bytes(w, h, guard, cell)
    assert z_bytes == 4 * ch * cw
    zbuf = torch.full((ch * cw + 16,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)  # not cleared: the entry point does
    keep = float(ref.keep_of(rho))
    _lib.check(lib.gsl_map_occl_depth(ptr(m_t), n, ptr(w_t), *intr, w, h, guard, cell, NEAR, FAR, ptr(zbuf), z_bytes,
                                      st), "gsl_map_occl_depth")
    _lib.check(lib.gsl_map_occl_select(ptr(m_t), n, ptr(w_t), *intr, w, h, guard, NEAR, FAR, cell, window, keep,
                                       ptr(zbuf), z_bytes, ptr(prev_ws), ptr(counters), ptr(ws), ws_bytes, st),
               "gsl_map_occl_select")
    first = counters.tolist()
    if gather:
        _lib.check(lib.gsl_map_view_gather(ptr(m_t), ptr(c_t), n, ptr(out_m), ptr(out_c), ptr(out_i), capacity,
                                           ptr(counters), ptr(ws), ws_bytes, st), "gsl_map_view_gather")
    torch.cuda.synchronize()
    assert bool((ws[ws_bytes:] == 0xAB).all())  # nothing behind the size the library asked for
    assert bool((zbuf[ch * cw:] == 0x5A5A5A5A).all())
    nb = (n + 255) // 256
    words = ws[:nb * 32].cpu().numpy().view(np.uint64)
    bits = ((words[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool).reshape(-1)
    assert not bits[n:].any()  # lanes past the last row select nothing
    return dict(first=first, counters=counters.tolist(), bits=bits[:n], ids=out_i.cpu().numpy(),
                means=out_m.cpu().numpy(), colors=out_c.cpu().numpy(), ws=ws,
                zbuf=zbuf[:ch * cw].cpu().numpy().view(np.uint32).reshape(ch, cw))


def _compare(means, colors, c2w, intr, w, h, cell, window, capacity=None):
    """One run against the mirror; returns (the mirror's result, the device's)."""
    n = means.shape[0]
    capacity = n + 3 if capacity is None else capacity
    w2c = ref.w2c_of(c2w)
    want = ref.select(means, w2c, intr, w, h, GUARD, NEAR, FAR, cell, window, RHO, out_capacity=capacity)
    got = _run(means, colors, w2c, intr, w, h, GUARD, cell, window, RHO, capacity)
    tag = (n, cell, window)
    assert np.array_equal(got["zbuf"], want["zbuf"]), tag
    sel, _, written, culled = want["counters"]
    assert got["first"] == [sel, 0, 0, culled], (tag, got["first"], want["counters"])
    assert tuple(got["counters"]) == want["counters"] == (sel, 0, min(sel, capacity), culled), tag
    assert np.array_equal(got["bits"], want["mask"]), tag
    gpu._check_outputs(got, want["ids"], means, colors, capacity)
    return want, got


@pytest.fixture(scope="module")
def cases():
    """Every (rows, scene) case, made once and left unchanged."""
    made = {}

    def get(n, scene):
        if (n, scene) not in made:
            means, c2w, intr, w, h = _case(n, scene)
            colors = np.random.default_rng(n).uniform(0.0, 1.0, (n, 3)).astype(F32)
            for a in (means, colors):
                a.setflags(write=False)
            made[(n, scene)] = (means, colors, c2w, intr, w, h)
        return made[(n, scene)]

    return get


@pytest.mark.parametrize("scene", SCENES)
@pytest.mark.parametrize("n", ROWS)
def test_depth_select_and_gather_against_the_mirror(n, scene, cases):
    means, colors, c2w, intr, w, h = cases(n, scene)
    for cell, window in PAIRS:
        want, _ = _compare(means, colors, c2w, intr, w, h, cell, window)
        sel, _, _, culled = want["counters"]
        band = int(want["band"].sum())
        assert sel + culled == band
        if scene == "two_walls" and n >= 4099 and (cell, window) == (4, 1):
            assert 4 * culled >= n and 4 * sel >= n, (n, sel, culled)
        if scene == "equal_depths" or (scene == "sparse" and cell <= 4 and window <= 1):
            assert culled == 0 and sel == band and (band == n or scene == "equal_depths"), (scene, n, cell, window)
        if scene.startswith("one_cell") and cell >= 4:
            assert (want["zbuf"] != 0).sum() == 1 and band == n  # one word takes every row
        if scene == "random" and n >= 1000:
            assert 0.1 < want["band"].mean() < 0.8


def test_the_runs_start_and_end_where_they_should(cases):
    """The scene is what it says, for the 4-pixel cells it was made for: the mirror's cells change exactly at the run
    boundaries, which lie at lanes 0, 31, 32, 33 of a wave, and runs span a wave and a workgroup boundary."""
    means, _, c2w, intr, w, h = cases(4099, "runs")
    z, u, v = ref.project(means, ref.w2c_of(c2w), intr)
    band = ref.in_band(z, u, v, w, h, GUARD, NEAR, FAR)
    assert band.all()
    gi, ch, cw = ref.grid(w, h, GUARD, 4)
    cu, cv = ref.cells(u, v, band, gi, 4)
    cell = cv * cw + cu
    starts = np.flatnonzero(np.diff(cell) != 0) + 1
    want = np.cumsum(np.resize(RUN_LENGTHS, 200))
    assert np.array_equal(starts, want[want < 4099])
    lanes = set((starts % 64).tolist())
    assert {0, 31, 32, 33} <= lanes  # a run ends at lane 63 where the next starts at lane 0, at 31 where it starts at 32
    ends = np.append(starts[1:], 4099) - 1
    assert any(s // 64 != e // 64 for s, e in zip(starts, ends)) and any(s // 256 != e // 256 for s, e in zip(starts, ends))


@pytest.mark.parametrize("scene", ["two_walls", "random"])
def test_every_cell_and_window(scene, cases):
    means, colors, c2w, intr, w, h = cases(4099, scene)
    culled = {}
    for cell in ref.CELLS:
        for window in range(4):
            culled[(cell, window)] = _compare(means, colors, c2w, intr, w, h, cell, window)[0]["counters"][3]
    print(f"[occl] {scene}, 4099 rows: culled per (cell_px, window) {culled}")
    if scene == "two_walls":
        assert all(culled[(cell, 0)] >= culled[(cell, 3)] for cell in ref.CELLS)  # a wider window only keeps more
        assert culled[(4, 1)] > 0


def test_a_shuffled_map_gives_the_same_buffer_and_the_same_rows(cases):
    for scene in ("two_walls", "runs", "one_cell_shuffled"):
        means, colors, c2w, intr, w, h = cases(4099, scene)
        n = means.shape[0]
        w2c = ref.w2c_of(c2w)
        a = _run(means, colors, w2c, intr, w, h, GUARD, 4, 1, RHO, n)
        again = _run(means, colors, w2c, intr, w, h, GUARD, 4, 1, RHO, n)
        assert np.array_equal(a["zbuf"], again["zbuf"]) and np.array_equal(a["bits"], again["bits"])
        assert a["counters"] == again["counters"] and np.array_equal(a["ids"], again["ids"])
        order = np.random.default_rng(5).permutation(n)
        b = _run(means[order], colors[order], w2c, intr, w, h, GUARD, 4, 1, RHO, n)
        assert np.array_equal(a["zbuf"], b["zbuf"]), scene
        k = b["counters"][2]
        assert b["counters"] == a["counters"]
        assert np.array_equal(np.sort(order[b["ids"][:k]]), a["ids"][:k]), scene  # the same rows, by original index


def test_violations_against_an_earlier_selection(cases):
    """Pose B against the ballots pose A left: the rows visible from B (its own z-buffer, the reach as guard) that A did
    not select.  4099 rows and 66 000 (two counts per thread of the three scans)."""
    for n in (4099, 66000):
        means, colors, c2w, intr, w, h = cases(n, "two_walls")
        pose_b = gpu._pose(39.0, (1.6, -0.8, 2.1))
        w2c_a, w2c_b = ref.w2c_of(c2w), ref.w2c_of(pose_b)
        a = _run(means, colors, w2c_a, intr, w, h, GUARD, 4, 1, RHO, n)
        mask_a = ref.select(means, w2c_a, intr, w, h, GUARD, NEAR, FAR, 4, 1, RHO)["mask"]
        assert np.array_equal(a["bits"], mask_a)
        before = a["ws"].clone()
        want = ref.select(means, w2c_b, intr, w, h, 4.0, NEAR, FAR, 4, 1, RHO, prev=mask_a)
        b = _run(means, colors, w2c_b, intr, w, h, 4.0, 4, 1, RHO, n, prev_ws=a["ws"], gather=False)
        sel, fresh, _, culled = want["counters"]
        assert fresh > 0 and culled > 0 and b["counters"] == [sel, fresh, 0, culled], (b["counters"], want["counters"])
        assert fresh == ref.violations(means, w2c_b, intr, w, h, 4.0, NEAR, FAR, 4, 1, RHO, mask_a)
        assert np.array_equal(b["bits"], want["mask"]) and np.array_equal(b["zbuf"], want["zbuf"])
        assert torch.equal(a["ws"], before)  # prev_ws is only read
        # some of the fresh rows were in A's band and culled there: parallax has uncovered them
        band_a = ref.select(means, w2c_a, intr, w, h, GUARD, NEAR, FAR, 4, 1, RHO)["band"]
        assert int((want["mask"] & ~mask_a & band_a).sum()) > 0


def test_a_gather_beyond_the_capacity_clamps(cases):
    means, colors, c2w, intr, w, h = cases(4099, "two_walls")
    sel = ref.select(means, ref.w2c_of(c2w), intr, w, h, GUARD, NEAR, FAR, 4, 1, RHO)["counters"][0]
    assert sel > 2
    for cap in (sel // 2, 0):
        want, got = _compare(means, colors, c2w, intr, w, h, 4, 1, capacity=cap)
        assert got["counters"][0] == sel and got["counters"][2] == cap


def test_gaussian_map_wraps_the_entry_points(cases):
    means, colors, pose_a, intr, w, h = cases(4099, "two_walls")
    n, cap = means.shape[0], 5000
    pose_b = gpu._pose(39.0, (1.6, -0.8, 2.1))
    m = GaussianMap(w, h, MapConfig(capacity=cap, view_guard_px=GUARD, view_reach_px=4.0, view_occlusion_rho=RHO), DEV)
    K = torch.tensor([[intr[0], 0.0, intr[2]], [0.0, intr[1], intr[3]], [0.0, 0.0, 1.0]])
    assert m.select_view(K, torch.from_numpy(pose_a), GUARD, NEAR, FAR, occlusion_rho=RHO)[3] == 0  # an empty map
    m.means[:n], m.colors[:n], m.n_live = torch.tensor(means, device=DEV), torch.tensor(colors, device=DEV), n
    f_intr = tuple(float(F32(a)) for a in intr)
    want = ref.select(means, ref.w2c_of(pose_a), f_intr, w, h, GUARD, NEAR, FAR, 4, 1, RHO)
    pts, col, ids, k = m.select_view(K, torch.from_numpy(pose_a).to(DEV), GUARD, NEAR, FAR, occlusion_rho=RHO)
    assert k == want["counters"][0] and 0 < k < n and m.last_view_culled == want["counters"][3] > 0
    assert np.array_equal(ids.cpu().numpy(), want["ids"])
    assert torch.equal(pts, m.means[ids.long()]) and torch.equal(col, m.colors[ids.long()])
    assert pts.data_ptr() == m._view["means"].data_ptr()  # the working buffers of the view
    assert m.view_violations(K, torch.from_numpy(pose_a), NEAR, FAR) == ref.violations(
        means, ref.w2c_of(pose_a), f_intr, w, h, 4.0, NEAR, FAR, 4, 1, RHO, want["mask"])
    v = m.view_violations(K, torch.from_numpy(pose_b), NEAR, FAR)
    assert v == ref.violations(means, ref.w2c_of(pose_b), f_intr, w, h, 4.0, NEAR, FAR, 4, 1, RHO, want["mask"]) > 0
    assert torch.equal(pts, m.means[ids.long()])  # the check gathers nothing
    depth, raw = m.view_depth(K, torch.from_numpy(pose_a), GUARD, NEAR, FAR)
    assert np.array_equal(raw.cpu().numpy().view(np.uint32), want["zbuf"])
    assert np.array_equal(depth.cpu().numpy().view(np.uint32), ref.depth_of(want["zbuf"]).view(np.uint32))
    assert len(m._occl["zbufs"]) == 2  # one per grid size: the guard's and the reach's, kept
    # without the option the same map selects with the frustum alone, and the check follows that rule
    k_all = m.select_view(K, torch.from_numpy(pose_a), GUARD, NEAR, FAR)[3]
    assert k_all == int(want["band"].sum()) and m.last_view_culled == 0
    assert m.view_violations(K, torch.from_numpy(pose_a), NEAR, FAR) == 0
    m.n_live = n - 1
    with pytest.raises(RuntimeError, match="select_view"):
        m.view_violations(K, torch.from_numpy(pose_a), NEAR, FAR)
