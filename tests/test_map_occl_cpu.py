"""Occlusion culling of the local map (csrc/map_occl.hip), the parts that need no GPU: the mirror of the rule on hand-made
cases, clause by clause; the conditions on the synthetic scenes that the GPU tests rely on, asserted with the mirror;
the byte functions and the argument checks of the entry points; MapConfig; and Localizer(mode="map") with
``view_occlusion_rho`` around the stand-in tracker / renderer of tests/test_map_cpu.py and a map whose device calls are
the mirrors.

The scenes (160x120, the intrinsics of the synthetic sequences):
  box room   the 16 ground-truth poses of the local-map sweep (1 degree, 1 cm, axis (0.3, 1, -0.2)), the back-projected
             points of frames 0, 5, 10 and 15: a room seen from inside hides nothing of itself, 0 rows culled;
  two views  a panel 1.0 x 0.8 m at z = 1.5 seen from x = -0.8 and x = +0.8, the points of both frames from the second:
             the first view's wall behind the panel is culled, and nothing that is not behind the second frame's depth."""
import ctypes

import numpy as np
import pytest
import torch

from gsplatloc_amd import _lib
from gsplatloc_amd.data import Parser
from gsplatloc_amd.mapping import GaussianMap, MapConfig
from gsplatloc_amd.my_gsplat import TrackerConfig
from gsplatloc_amd.my_gsplat.geometry import depth_to_points
from gsplatloc_amd.synthetic import (_twist, panel_depth, replica_intrinsics, room_depth, write_replica_passing_panel)
from tests import map_occl_ref as ref
from tests import test_map_cpu as base
from tests import test_map_view_cpu as view
from tests.test_abi import prototypes

F32 = np.float32
NEAR, FAR = TrackerConfig().gs.near_plane, TrackerConfig().gs.far_plane

# ---- the mirror of the rule: power-of-two intrinsics, u = 64 x / z + 32 and v = 64 y / z + 24 exact for dyadic rows ----
RW, RH, INTR, G = 64, 48, (64.0, 64.0, 32.0, 24.0), 8.0
EYE = np.eye(4, dtype=F32)


def _at(u, v, z):
    """The camera-frame point that projects onto (u, v) at the depth z."""
    return [(u - 32.0) / 64.0 * z, (v - 24.0) / 64.0 * z, z]


def _select(points, cell=4, window=1, rho=0.25, guard=G, **kw):
    return ref.select(np.array(points, F32).reshape(-1, 3), EYE, INTR, RW, RH, guard, 0.5, 8.0, cell, window, rho, **kw)


def _block(u0, v0, z, cells=3, cell=4):
    """One row in the middle of every cell of a cells x cells block whose first cell starts at pixel (u0, v0)."""
    return [_at(u0 + cell * i + 2.0, v0 + cell * j + 2.0, z) for j in range(cells) for i in range(cells)]


def test_grid_and_cells():
    assert ref.grid(RW, RH, G, 4) == (8, 16, 20) and ref.grid(RW, RH, 7.25, 4) == (8, 16, 20)
    assert ref.grid(RW, RH, 0.0, 16) == (0, 3, 4) and ref.grid(160, 120, 8.0, 1) == (8, 136, 176)
    r = _select([_at(0.0, 0.0, 1.0), _at(3.75, 3.75, 2.0), _at(4.0, 0.0, 1.0)])
    assert r["zbuf"].shape == (16, 20) and r["zbuf"].dtype == np.uint32
    # (0, 0) and (3.75, 3.75) share the cell (2, 2): the nearer depth stays; (4, 0) is the next cell
    depth = ref.depth_of(r["zbuf"])
    assert depth[2, 2] == 1.0 and depth[2, 3] == 1.0 and np.isinf(depth).sum() == 16 * 20 - 2
    assert r["zbuf"][2, 2] == ~np.array([1.0], F32).view(np.uint32)[0]


def test_a_full_window_of_nearer_cells_culls_and_an_empty_cell_keeps():
    wall, behind = _block(8.0, 8.0, 1.0), _at(14.0, 14.0, 2.0)  # behind the middle cell of the block
    r = _select(wall + [behind])
    assert r["culled"].tolist() == [False] * 9 + [True] and r["counters"] == (9, 0, 9, 1)
    assert r["mask"].tolist() == [True] * 9 + [False] and r["ids"].tolist() == list(range(9))
    for gone in range(9):  # any one cell of the window empty (the middle one: only the row itself is there): kept
        if gone == 4:
            continue
        rows = [p for i, p in enumerate(wall) if i != gone] + [behind]
        assert _select(rows)["counters"] == (9, 0, 9, 0), gone
    # a row behind a corner cell of the block has empty cells in its window
    assert _select(wall + [_at(10.0, 10.0, 2.0)])["counters"][3] == 0


def test_a_cell_outside_the_grid_keeps_a_row():
    """The block in the grid's corner: the row behind the corner cell has a full window of nearer cells as far as the
    grid goes, and the cells beyond the grid count as empty.  One cell further in, it goes."""
    wall = _block(-8.0, -8.0, 1.0)  # cells (0..2, 0..2)
    assert _select(wall + [_at(-6.0, -6.0, 2.0)])["counters"] == (10, 0, 10, 0)
    assert _select(wall + [_at(-2.0, -2.0, 2.0)])["counters"] == (9, 0, 9, 1)
    far_corner = _block(RW - 1 + 8.0 - 11.0, RH - 1 + 8.0 - 11.0, 1.0)  # cells (17..19, 13..15): the last ones
    r = _select(far_corner + [_at(RW - 1 + 8.0 - 1.0, RH - 1 + 8.0 - 1.0, 2.0)])
    assert r["counters"] == (10, 0, 10, 0) and r["zbuf"][15, 19] != 0 and r["zbuf"][13, 17] != 0


def test_the_threshold_is_strict():
    """keep z == the stored depth keeps the row; one float32 step of z further: culled.  rho = 0.25: keep = 0.75."""
    wall = _block(8.0, 8.0, 1.5)
    on = _at(14.0, 14.0, 2.0)  # 0.75 * 2 == 1.5
    assert F32(0.75) * F32(2.0) == F32(1.5)
    assert _select(wall + [on])["counters"][3] == 0
    z = float(np.nextafter(F32(2.0), F32(3.0)))
    assert F32(0.75) * F32(z) > F32(1.5)
    assert _select(wall + [_at(14.0, 14.0, z)])["counters"][3] == 1
    assert ref.keep_of(0.05) == F32(1.0) - F32(0.05) and ref.keep_of(0.05).dtype == F32


def test_a_lone_row_in_front_of_a_wall():
    """window 1: nothing goes.  window 0: exactly the wall's rows of the lone row's own cell that lie behind it."""
    wall = [_at(8.0 + i + 0.5, 8.0 + j + 0.5, 2.0) for j in range(12) for i in range(12)]  # 9 cells, 16 rows each
    lone = _at(14.0, 14.0, 1.0)
    r1 = _select(wall + [lone], window=1)
    assert r1["counters"] == (145, 0, 145, 0)
    r0 = _select(wall + [lone], window=0)
    cu, cv = np.arange(12) // 4, np.arange(12) // 4
    own = ((cv[:, None] == 1) & (cu[None, :] == 1)).reshape(-1)
    assert r0["culled"].tolist() == own.tolist() + [False] and r0["counters"] == (145 - 16, 0, 145 - 16, 16)


def test_equal_depths_cull_nothing():
    rows = _block(8.0, 8.0, 2.0) + _block(8.0, 8.0, 2.0)
    for window in range(4):
        assert _select(rows, window=window)["counters"] == (18, 0, 18, 0)


def test_nan_and_inf_rows_never_enter_the_buffer_and_are_never_selected():
    nan, inf = np.nan, np.inf
    bad = [[nan, 0.0, 1.0], [0.0, nan, 1.0], [0.0, 0.0, nan], [inf, 0.0, 1.0], [0.0, -inf, 1.0], [0.0, 0.0, inf],
           [0.0, 0.0, -inf], [inf, inf, inf], [nan, nan, nan], [0.0, 0.0, -1.0], [0.0, 0.0, 0.25]]
    r = _select(bad + [_at(10.0, 10.0, 1.0)])
    assert r["band"].tolist() == [False] * len(bad) + [True] and r["mask"].tolist() == r["band"].tolist()
    assert (r["zbuf"] != 0).sum() == 1 and r["counters"] == (1, 0, 1, 0)
    assert (_select(bad)["zbuf"] == 0).all() and _select(bad)["counters"] == (0, 0, 0, 0)


def test_rows_on_the_borders_of_the_band_fall_into_the_first_and_last_cells():
    for cell in ref.CELLS:
        gi, ch, cw = ref.grid(RW, RH, G, cell)
        rows = [_at(-G, 10.0, 1.0), _at(RW - 1 + G, 10.0, 1.0), _at(10.0, -G, 1.0), _at(10.0, RH - 1 + G, 1.0),
                _at(-G, -G, 1.0), _at(RW - 1 + G, RH - 1 + G, 1.0)]
        r = _select(rows, cell=cell)
        assert r["band"].all(), cell
        z, u, v = ref.project(np.array(rows, F32), EYE, INTR)
        cu, cv = ref.cells(u, v, r["band"], gi, cell)
        assert cu.tolist() == [0, cw - 1, (10 + gi) // cell, (10 + gi) // cell, 0, cw - 1], cell
        assert cv.tolist() == [(10 + gi) // cell, (10 + gi) // cell, 0, ch - 1, 0, ch - 1], cell
    # a guard that is no whole number: gi = ceil(guard), the left border lies inside cell 0
    r = _select([_at(-7.25, 0.0, 1.0), _at(RW - 1 + 7.25, 0.0, 1.0), _at(-7.5, 0.0, 1.0)], guard=7.25)
    assert r["band"].tolist() == [True, True, False] and r["zbuf"][2, 0] != 0 and r["zbuf"][2, 19] != 0


def test_compaction_clamp_and_violation_count():
    wall, behind, aside = _block(8.0, 8.0, 1.0), _at(14.0, 14.0, 2.0), _at(40.0, 30.0, 2.0)
    rows = [behind] + wall + [aside, [0.0, 0.0, -1.0]]
    r = _select(rows)
    assert r["ids"].tolist() == list(range(1, 11)) and r["ids"].dtype == np.int32 and r["counters"] == (10, 0, 10, 1)
    assert _select(rows, out_capacity=4)["ids"].tolist() == [1, 2, 3, 4]
    assert _select(rows, out_capacity=4)["counters"] == (10, 0, 4, 1) and _select(rows, out_capacity=0)["counters"][2] == 0
    prev = np.zeros(12, bool)
    prev[[1, 2, 10]] = True
    assert _select(rows, prev=prev)["counters"] == (10, 7, 10, 1)
    # a z-buffer that is given is used as it is: an empty one culls nothing
    assert _select(rows, zb=np.zeros((16, 20), np.uint32))["counters"] == (11, 0, 11, 0)
    # seen from a camera 0.25 m to the right the row behind the wall is uncovered: a violation against the selection
    # above; the wall's rows, selected then, are none; a row occluded from both poses is none either
    moved = EYE.copy()
    moved[0, 3] = -0.25
    pts = np.array(rows, F32)
    args = (moved, INTR, RW, RH, 4.0, 0.5, 8.0, 4, 1, 0.25)
    there = ref.select(pts, *args)
    assert there["band"][0] and not there["culled"][0]
    assert ref.violations(pts, *args, prev=r["mask"]) == 1
    assert ref.violations(pts, EYE, INTR, RW, RH, 4.0, 0.5, 8.0, 4, 1, 0.25, prev=r["mask"]) == 0


# ---- the scenes ------------------------------------------------------------------------------------------------------
W, H = 160, 120


def _intr(w=W, h=H):
    K = replica_intrinsics(w, h)
    return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])


def _world(depth, c2w, w=W, h=H):
    p = depth_to_points(depth, replica_intrinsics(w, h)).numpy().astype(np.float64)
    return (p @ c2w[:3, :3].T + c2w[:3, 3]).astype(F32)


@pytest.fixture(scope="module")
def box_room():
    step, poses = _twist(1.0, 0.01, (0.3, 1.0, -0.2), (0.6, 0.1, 0.8)), [np.eye(4)]
    for _ in range(15):
        poses.append(poses[-1] @ step)
    K = replica_intrinsics(W, H)
    pts = np.concatenate([_world(room_depth(W, H, K, torch.from_numpy(poses[i]).float()), poses[i])
                          for i in (0, 5, 10, 15)])
    return pts, poses


@pytest.mark.parametrize("cell", [2, 4, 8])
def test_a_room_seen_from_inside_culls_nothing(box_room, cell):
    pts, poses = box_room
    assert pts.shape == (4 * W * H, 3) and len(poses) == 16
    defaults = MapConfig(view_guard_px=8.0, view_occlusion_rho=0.05)
    assert (defaults.view_occlusion_cell_px, defaults.view_occlusion_window) == (4, 1)
    for p in poses:
        r = ref.select(pts, ref.w2c_of(p), _intr(), W, H, 8.0, NEAR, FAR, cell, 1, 0.05)
        assert r["counters"][3] == 0 and r["counters"][0] == int(r["band"].sum()) > W * H


def _camera_at(x):
    c2w = np.eye(4)
    c2w[0, 3] = x
    return c2w


@pytest.fixture(scope="module")
def two_views():
    K, kw = replica_intrinsics(W, H), dict(center=(0.0, 0.0), size=(1.0, 0.8), z=1.5)
    a, b = _camera_at(-0.8), _camera_at(0.8)
    depth_a = panel_depth(W, H, K, torch.from_numpy(a).float(), **kw)
    depth_b = panel_depth(W, H, K, torch.from_numpy(b).float(), **kw)
    pts = np.concatenate([_world(depth_a, a), _world(depth_b, b)])
    z, u, v = ref.project(pts, ref.w2c_of(b), _intr())
    ui, vi = np.rint(u).astype(np.int64), np.rint(v).astype(np.int64)
    inside = (ui >= 0) & (ui < W) & (vi >= 0) & (vi < H)
    seen = np.full(len(pts), np.inf)
    seen[inside] = depth_b.numpy()[vi[inside], ui[inside]]  # the second frame's own depth at the row's pixel
    return pts, b, z, inside, seen


def test_the_wall_behind_a_panel_is_culled_and_nothing_else(two_views):
    pts, b, z, inside, seen = two_views
    r = ref.select(pts, ref.w2c_of(b), _intr(), W, H, 8.0, NEAR, FAR, 4, 1, 0.05)
    culled = r["culled"]
    print(f"[occl] two views: {int(r['band'].sum())} rows in the band, {int(culled.sum())} culled, "
          f"{int((r['band'] & inside & (z > 1.1 * seen)).sum())} more than 10 % behind the frame's depth")
    assert int(culled.sum()) >= 1500
    # every culled row is more than rho behind the frame's own depth at its pixel
    assert inside[culled].all() and (z[culled].astype(np.float64) * (1.0 - 0.05) > seen[culled]).all()


def test_a_window_of_zero_culls_rows_that_are_visible(two_views):
    """The regression test of the default window: with window 0 a slanted surface culls its own far side within a cell,
    and rows that are NOT behind the frame's depth go."""
    pts, b, z, inside, seen = two_views
    r = ref.select(pts, ref.w2c_of(b), _intr(), W, H, 8.0, NEAR, FAR, 4, 0, 0.05)
    culled = r["culled"]
    false_culls = culled & ~(inside & (z.astype(np.float64) * (1.0 - 0.05) > seen))
    print(f"[occl] two views, window 0: {int(culled.sum())} culled, {int(false_culls.sum())} of them not behind the "
          "frame's depth")
    assert int(false_culls.sum()) > 0


# ---- the entry points -------------------------------------------------------------------------------------------------
BAD_ARG, WORKSPACE = -1, -2
_DEPTH = dict(n_rows=1000, fx=50.0, fy=40.0, cx=31.5, cy=23.5, width=64, height=48, guard_px=8.0, cell_px=4,
              near_plane=0.01, far_plane=100.0, zbuf_bytes="zfull")
_SELECT = dict(_DEPTH, window=1, rho_keep=0.95, prev_ws=None, ws_bytes="full")
D, S = "gsl_map_occl_depth", "gsl_map_occl_select"
_COMMON = [
    ("NULL means", dict(means=None), BAD_ARG), ("NULL w2c", dict(w2c=None), BAD_ARG),
    ("NULL zbuf", dict(zbuf=None), BAD_ARG),
    ("n_rows == 0", dict(n_rows=0), BAD_ARG), ("n_rows < 0", dict(n_rows=-5), BAD_ARG),
    ("n_rows == 2^31", dict(n_rows=1 << 31), BAD_ARG), ("n_rows beyond 2^32", dict(n_rows=(1 << 32) + 7), BAD_ARG),
    ("width <= 0", dict(width=0), BAD_ARG), ("height <= 0", dict(height=-3), BAD_ARG),
    ("width * height > 2^31 - 1", dict(width=1 << 16, height=1 << 15), BAD_ARG),
    ("fx == 0", dict(fx=0.0), BAD_ARG), ("fy == 0", dict(fy=0.0), BAD_ARG),
    ("negative guard", dict(guard_px=-0.5), BAD_ARG), ("NaN guard", dict(guard_px=float("nan")), BAD_ARG),
    ("a guard without end", dict(guard_px=float("inf")), BAD_ARG),
    ("negative near", dict(near_plane=-0.01), BAD_ARG), ("NaN near", dict(near_plane=float("nan")), BAD_ARG),
    ("near == far", dict(near_plane=2.0, far_plane=2.0), BAD_ARG),
    ("near > far", dict(near_plane=3.0, far_plane=2.0), BAD_ARG),
    ("cell 0", dict(cell_px=0), BAD_ARG), ("cell 3", dict(cell_px=3), BAD_ARG), ("cell 32", dict(cell_px=32), BAD_ARG),
    ("cell -4", dict(cell_px=-4), BAD_ARG),
    ("more than 2^26 cells", dict(width=16384, height=8192, cell_px=1, guard_px=0.0), BAD_ARG),
    ("zbuf one byte short", dict(zbuf_bytes="zshort"), WORKSPACE), ("zbuf of 8 bytes", dict(zbuf_bytes=8), WORKSPACE),
]
_ONLY_SELECT = [
    ("NULL counters", dict(counters=None), BAD_ARG), ("NULL ws", dict(ws=None), BAD_ARG),
    ("window -1", dict(window=-1), BAD_ARG), ("window 4", dict(window=4), BAD_ARG),
    ("keep 0", dict(rho_keep=0.0), BAD_ARG), ("keep 1", dict(rho_keep=1.0), BAD_ARG),
    ("keep NaN", dict(rho_keep=float("nan")), BAD_ARG), ("keep -0.5", dict(rho_keep=-0.5), BAD_ARG),
    ("prev_ws == ws", dict(prev_ws="buffer"), BAD_ARG),
    ("short workspace", dict(ws_bytes=8), WORKSPACE), ("workspace one byte short", dict(ws_bytes="short"), WORKSPACE),
    ("the view's workspace is too small", dict(ws_bytes="view"), WORKSPACE),
]


def test_byte_functions():
    lib = _lib.load_library()
    # per 256-row workgroup: four 64-bit ballots, three counts and their three bases
    assert lib.gsl_map_occl_ws_bytes(1) == 56 and lib.gsl_map_occl_ws_bytes(256) == 56
    assert lib.gsl_map_occl_ws_bytes(257) == 112 and lib.gsl_map_occl_ws_bytes(1_000_000) == 3907 * 56
    assert lib.gsl_map_occl_ws_bytes((1 << 31) - 1) == (1 << 23) * 56
    assert lib.gsl_map_occl_ws_bytes(0) == 56 and lib.gsl_map_occl_ws_bytes(1 << 31) == 56
    for n in (1, 257, 66000):  # the gather reads the same workspace: never smaller than the view's
        assert lib.gsl_map_occl_ws_bytes(n) >= lib.gsl_map_view_ws_bytes(n)
    z = lib.gsl_map_occl_zbuf_bytes
    for w, h, guard, cell in ((64, 48, 8.0, 4), (64, 48, 7.25, 4), (160, 120, 8.0, 1), (1200, 680, 8.0, 4),
                              (1200, 680, 0.0, 16), (1, 1, 0.0, 16), (160, 120, 4.0, 2), (161, 119, 0.5, 8)):
        gi, ch, cw = ref.grid(w, h, guard, cell)
        assert z(w, h, guard, cell) == 4 * ch * cw, (w, h, guard, cell)
    assert z(1200, 680, 8.0, 4) == 4 * 174 * 304  # about 200 KB: it lives in L2
    assert z(8192, 8192, 0.0, 1) == 4 << 26 and z(8193, 8192, 0.0, 1) == 0  # 2^26 cells and one column more
    for bad in ((0, 48, 8.0, 4), (64, -1, 8.0, 4), (64, 48, -1.0, 4), (64, 48, float("nan"), 4), (64, 48, 8.0, 3),
                (64, 48, 8.0, 0), (64, 48, 8.0, 32), (64, 48, float("inf"), 4), (64, 48, 3e7, 16),
                (1 << 16, 1 << 15, 0.0, 16), ((1 << 24) + 1, 1, 0.0, 16)):
        assert z(*bad) == 0, bad


@pytest.mark.parametrize("fn", [D, S])
def test_entry_points_reject_bad_arguments_before_any_launch(fn, repo_root):
    """Every row is refused on the host: the pointers are one dummy HOST buffer, a launch would give GSL_ERR_HIP or
    worse."""
    lib = _lib.load_library()
    params = prototypes(repo_root)[fn][1]
    buf = ctypes.create_string_buffer(256)
    rows = _COMMON + (_ONLY_SELECT if fn == S else [])
    for what, over, want in rows:
        named = dict(_SELECT if fn == S else _DEPTH, **over)
        assert set(named) <= {n for _, n in params}, (fn, what)
        full = lib.gsl_map_occl_ws_bytes(named["n_rows"])
        zfull = lib.gsl_map_occl_zbuf_bytes(named["width"], named["height"], named["guard_px"], named["cell_px"])
        words = {"full": full, "short": full - 1, "view": lib.gsl_map_view_ws_bytes(named["n_rows"]), "zfull": zfull,
                 "zshort": zfull - 1, "buffer": ctypes.addressof(buf)}
        args = []
        for c_type, name in params:
            if name == "stream":
                args.append(None)
            elif name in named:
                args.append(words[named[name]] if isinstance(named[name], str) else named[name])
            else:
                args.append(ctypes.addressof(buf) if "*" in c_type else 0)
        assert getattr(lib, fn)(*args) == want, (fn, what)
    assert not any(buf.raw)  # nothing wrote to the buffer


def test_map_config_validation():
    c = MapConfig()
    assert (c.view_occlusion_rho, c.view_occlusion_cell_px, c.view_occlusion_window) == (None, 4, 1)
    c = MapConfig(view_guard_px=8.0, view_occlusion_rho=0.05, view_occlusion_cell_px=16, view_occlusion_window=3)
    assert c.view_occlusion_rho == 0.05
    for kw in (dict(view_occlusion_rho=0.05), dict(view_guard_px=8.0, view_occlusion_rho=0.0),
               dict(view_guard_px=8.0, view_occlusion_rho=1.0), dict(view_guard_px=8.0, view_occlusion_rho=-0.1),
               dict(view_guard_px=8.0, view_occlusion_rho=float("nan")), dict(view_guard_px=8.0, view_occlusion_rho=True),
               dict(view_occlusion_cell_px=3), dict(view_occlusion_cell_px=0), dict(view_occlusion_cell_px=32),
               dict(view_occlusion_cell_px=4.0), dict(view_occlusion_window=-1), dict(view_occlusion_window=4),
               dict(view_occlusion_window=1.0)):
        with pytest.raises(ValueError, match="view_occlusion"):
            MapConfig(**kw)
    m = GaussianMap(32, 24, MapConfig(view_guard_px=8.0, view_occlusion_rho=0.05), "cpu")
    assert m.occlusion_grid(8.0) == ref.grid(32, 24, 8.0, 4) and m.last_view_culled == 0
    K = replica_intrinsics(32, 24)
    assert m.select_view(K, torch.eye(4), 8.0, NEAR, FAR, occlusion_rho=0.05)[3] == 0  # an empty map: no launch
    depth, raw = m.view_depth(K, torch.eye(4), 8.0, NEAR, FAR)
    assert depth.shape == raw.shape == (10, 12) and bool(torch.isinf(depth).all()) and not bool(raw.any())
    m.n_live = 3
    with pytest.raises(AssertionError, match="no CPU path"):
        m.select_view(K, torch.eye(4), 8.0, NEAR, FAR, occlusion_rho=0.05)
    with pytest.raises(ValueError, match="occlusion_rho"):
        m.select_view(K, torch.eye(4), 8.0, NEAR, FAR, occlusion_rho=1.5)


# ---- Localizer(mode="map", view_occlusion_rho) around stand-ins -----------------------------------------------------
LW, LH, N_OUT, STEP = 32, 24, 4, 0.15
GUARD, REACH, CELL, WINDOW, RHO = 4.0, 1.0, 1, 1, 0.05


class _OcclMirrorMap(view._ViewMirrorMap):
    """The view test's mirror map with the occlusion launch as the numpy mirror as well; records those calls."""
    occl_calls = []

    def _occl_launch(self, intr, w2c, guard_px, near, far, check, rho):
        v = self._view_buffers()
        r = ref.select(self.means[:self.n_live].numpy(), w2c.numpy(), intr, self.W, self.H, guard_px, near, far,
                       self.cfg.view_occlusion_cell_px, self.cfg.view_occlusion_window, rho, out_capacity=self.capacity,
                       prev=self._occl_mask if check else None)
        _OcclMirrorMap.occl_calls.append(dict(check=check, w2c=w2c.numpy().copy(), guard=guard_px, near=near, far=far,
                                              rho=rho, counters=r["counters"]))
        if not check:
            self._occl_mask, ids = r["mask"], torch.from_numpy(r["ids"]).long()
            v["means"][:len(ids)], v["colors"][:len(ids)] = self.means[ids], self.colors[ids]
            v["ids"][:len(ids)] = torch.from_numpy(r["ids"])
        return r["counters"]


@pytest.fixture(scope="module")
def passing(tmp_path_factory):
    """The camera passes the panel and comes back: 2 N_OUT + 1 frames at 32x24."""
    root = tmp_path_factory.mktemp("occl_seq")
    poses = write_replica_passing_panel(root, LW, LH, N_OUT + 1, step=STEP, and_back=True)
    assert poses.shape[0] == 2 * N_OUT + 1 and torch.equal(poses[0], poses[-1])
    parser = Parser("Replica", "room0", normalize=False, device="cpu", input_folder=str(root))
    return [parser.frame(i) for i in range(2 * N_OUT + 1)]


def _localizer(config, factory):
    view._ViewMirrorMap.view_calls, view._ViewMirrorMap.renders, _OcclMirrorMap.occl_calls = [], [], []
    return view._localizer(base._Tracker, base._Renderer(), False, config, map_factory=factory)


def test_occlusion_mode_tracks_the_visible_rows_and_repairs_what_parallax_uncovers(passing):
    config = MapConfig(view_guard_px=GUARD, view_reach_px=REACH, view_occlusion_rho=RHO, view_occlusion_cell_px=CELL,
                       view_occlusion_window=WINDOW)
    loc = _localizer(config, _OcclMirrorMap)
    loc.reset(*passing[0])
    geom = (_intr(LW, LH), LW, LH)
    rule = (CELL, WINDOW, RHO)
    culled, violations = [], []
    for k in range(1, len(passing)):
        prefix, start = loc.map.points.numpy().copy(), loc.trajectory[k - 1].numpy().copy()
        _OcclMirrorMap.occl_calls = []
        r = loc.track(passing[k][0], passing[k][1], gt_c2w=passing[k][2])
        want = ref.select(prefix, ref.w2c_of(start), *geom, GUARD, NEAR, FAR, *rule)
        load = base._Tracker.made[-1].loads[-1]
        assert r.tracked == want["counters"][0] == load["tar_points"].shape[0] and not r.lost
        assert r.view_culled == want["counters"][3] == int(want["band"].sum()) - r.tracked
        assert torch.equal(load["tar_points"], torch.from_numpy(prefix[want["mask"]]))
        est = ref.w2c_of(r.c2w.numpy())
        assert r.view_violations == ref.violations(prefix, est, *geom, REACH, NEAR, FAR, *rule, prev=want["mask"])
        calls = _OcclMirrorMap.occl_calls
        assert [c["check"] for c in calls] == [False, True] + ([False] if r.view_violations else [])
        assert [c["guard"] for c in calls] == [GUARD, REACH] + ([GUARD] if r.view_violations else [])
        assert all(c["rho"] == RHO and c["near"] == NEAR and c["far"] == FAR for c in calls)
        assert np.array_equal(calls[0]["w2c"], ref.w2c_of(start)) and all(np.array_equal(c["w2c"], est) for c in calls[1:])
        if r.view_violations:  # the insertion render is of a new selection at the estimate, which holds the rows
            again = ref.select(prefix, est, *geom, GUARD, NEAR, FAR, *rule)
            assert calls[2]["counters"] == again["counters"]
            assert torch.equal(loc._render_map.calls[-1]["points"], torch.from_numpy(prefix[again["mask"]]))
            assert not (ref.select(prefix, est, *geom, REACH, NEAR, FAR, *rule)["mask"] & ~again["band"]).any()
        culled.append(r.view_culled)
        violations.append(r.view_violations)
    assert view._ViewMirrorMap.view_calls == []  # every selection went through the occlusion rule
    print(f"[occl] stand-in flow: culled {culled}, violations {violations}")
    assert max(culled) > 0 and any(c > 0 for c in culled[:N_OUT])
    # on the way back parallax uncovers what was culled: violations, repaired by a selection at the estimate
    assert any(v > 0 for v in violations[N_OUT:]), violations


def test_without_the_option_the_calls_are_those_of_the_view_mode(passing):
    """view_occlusion_rho=None: the calls on the map, the tracker's loads and the rows inserted are those of a map
    without the occlusion entry points (the view test's mirror map); the occlusion launch is never made."""
    runs = []
    for factory in (view._ViewMirrorMap, _OcclMirrorMap):
        loc = _localizer(MapConfig(view_guard_px=GUARD, view_reach_px=REACH), factory)
        loc.reset(*passing[0])
        results = [loc.track(f[0], f[1], gt_c2w=f[2]) for f in passing[1:]]
        assert _OcclMirrorMap.occl_calls == [] and all(r.view_culled is None for r in results)
        assert loc.map._occl is None and loc.map.last_view_culled == 0
        loads = [t.loads[-1] for t in base._Tracker.made]
        runs.append((view._ViewMirrorMap.view_calls, loads, loc.map.points.clone(), loc.trajectory.clone(),
                     [(r.tracked, r.view_violations, r.added) for r in results]))
    (calls_a, loads_a, points_a, traj_a, res_a), (calls_b, loads_b, points_b, traj_b, res_b) = runs
    assert len(calls_a) == len(calls_b) >= 2 * (len(passing) - 1) and res_a == res_b
    for a, b in zip(calls_a, calls_b):
        assert a.keys() == b.keys() and all(np.array_equal(a[name], b[name]) for name in a)
    assert len(loads_a) == len(loads_b)
    for a, b in zip(loads_a, loads_b):
        assert all((a[name] is None and b[name] is None) or torch.equal(a[name], b[name]) for name in a)
    assert torch.equal(points_a, points_b) and torch.equal(traj_a, traj_b)


def test_the_kernels_cost_what_the_documents_say():
    """hipcc's resource remarks (no GPU needed): the figures of the kernel table in DESIGN.md 4, and the one variant of
    the depth kernel that the library is built with -- the lanes of a wave combined, no load in front of the atomic."""
    from tests.test_kernel_resources import HIPCC, _resources
    import os

    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    found = _resources("map_occl.hip")
    depth = [v for k, v in found.items() if "k_map_occl_depth" in k]
    assert len(depth) == 1 and [k for k in found if "k_map_occl_depthILb0ELb1E" in k]
    select = [v for k, v in found.items() if "k_map_occl_select" in k][0]
    for r, vgprs, sgprs, lds in ((depth[0], 15, 38, 0), (select, 14, 52, 48)):
        assert r["VGPRs"] <= vgprs and r["AGPRs"] == 0 and r["TotalSGPRs"] <= sgprs, r
        assert r["LDS"] <= lds and r["ScratchSize"] == 0 and r["Occupancy"] == 8, r
