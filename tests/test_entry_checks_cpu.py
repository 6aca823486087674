"""Status of the fused pipeline's entry points for calls that return before any launch (no GPU needed).

The host code in front of every launch is a ladder of argument checks; which status a call gets when two of them could
fire (GSL_ERR_BAD_ARG against GSL_ERR_WORKSPACE) depends on their order.  The table below pins, per entry point: every
geometry condition violated alone, a NULL required pointer, ``ed`` with three channels, a short workspace together
with a bad argument, and the early GSL_OK returns.  The expected column was recorded from the library as it was before
the entry points were moved to one file per stage and given a shared frame check; it is not derived from the code.

No row may reach a launch -- the pointers are dummy HOST buffers (the entry points do not dereference on the host).
Every row therefore either keeps its entry point's early-return guard (an empty strip, capacity 0, N = 0) or is the
row that tests that guard, or fails a check that sits in front of the first launch.  Entry points without a workspace
argument (or whose workspace check can only be reached past the guard) have no workspace rows.
"""
import ctypes

import pytest

from gsplatloc_amd import _lib
from tests.test_abi import prototypes

OK, BAD_ARG, WORKSPACE, ERR_HIP = 0, -1, -2, -3

# 64 x 48 frame, 4 x 3 tiles of 16 pixels, RGB + expected depth
_FRAME = dict(width=64, height=48, tile_w=4, tile_h=3, channels=4, ed=1)
_STRIP = dict(ty0=0, ty1=0, row0=0, row1=48, capacity=100)  # ty0 == ty1: the empty strip every raster entry returns on
_FULL = "full"  # stands for "the size the library asks for" in a *_bytes argument

# entry point -> arguments of a valid call that returns GSL_OK before its first launch (pointers not named: dummies)
BASE = {
    "gsl_fused_raster_fwd": dict(_FRAME, **_STRIP, long_min=0, sort_bins=None, bin_cap=0),
    "gsl_long_raster_fwd": dict(_FRAME, **_STRIP, long_min=512, max_seg=8, long_ws_bytes=_FULL, map_ready=0),
    "gsl_fused_raster_bwd": dict(_FRAME, **_STRIP, long_min=0, vrow=None, clear_ws=None),
    "gsl_long_raster_bwd": dict(_FRAME, **_STRIP, long_min=512, max_seg=8),
    "gsl_tiny_raster_bwd": dict(_FRAME, **_STRIP, long_min=0, loss_depth_gt=None, clear_ws=None),
    "gsl_fused_absgrad": dict(_FRAME, capacity=0),
    # N = 0 in binned mode: nothing to project, and the sort kernel (gsl_fused_bin) adds up the tile sizes
    "gsl_fused_project": dict(width=64, height=48, tile_w=4, tile_h=3, ty0=0, ty1=3, N=0, sh_degree=0, K_sh=1,
                              antialiased=0, bin_cap=64, ws_bytes=_FULL, eps2d=0.3, near_plane=0.01, far_plane=1e10),
    "gsl_fused_bin": dict(tile_w=4, tile_h=3, ty0=0, ty1=3, N=0, capacity=0, bins=None, bin_cap=0, ws_bytes=_FULL,
                          write_sorted_keys=0, long_min=0),
    "gsl_fused_project_bwd": dict(width=64, height=48, n_tiles=12, tile_w=4, tile_h=3, ty0=0, ty1=3, N=0, channels=4,
                                  sh_degree=0, K_sh=1, antialiased=0, reduce_viewmat=0, capacity=100, vrow=None,
                                  tiny_trec=None, ws_bytes=_FULL, eps2d=0.3),
}

_GEOMETRY = [  # the frame conditions of the compositing entry points, each violated alone
    ("width <= 0", dict(width=0)), ("height <= 0", dict(height=0)), ("tile_w <= 0", dict(tile_w=0)),
    ("tile_h <= 0", dict(tile_h=0)), ("ty0 < 0", dict(ty0=-1, ty1=-1)), ("ty1 > tile_h", dict(ty0=4, ty1=4)),
    ("ty0 > ty1", dict(ty0=1, ty1=0)), ("capacity < 0", dict(capacity=-1)), ("row0 < 0", dict(row0=-1)),
    ("row0 > row1", dict(row0=10, row1=5)), ("tile_w * 16 < width", dict(width=65)),
    ("tile_h * 16 < height", dict(height=49)),
]
_SHORT_WS = dict(N=256, reduce_viewmat=0, ws_bytes=0)  # gsl_fused_project_bwd checks its workspace last, behind N == 0


def _rows():
    rows = []
    for fn in ("gsl_fused_raster_fwd", "gsl_fused_raster_bwd", "gsl_tiny_raster_bwd"):
        rows += [(fn, what, over, BAD_ARG) for what, over in _GEOMETRY]
    # the long-list entry points have never asked that the tile grid cover the frame
    for fn in ("gsl_long_raster_fwd", "gsl_long_raster_bwd"):
        rows += [(fn, what, over, OK if "* 16 <" in what else BAD_ARG) for what, over in _GEOMETRY]
        rows += [(fn, "long_min <= 0", dict(long_min=0), BAD_ARG), (fn, "max_seg <= 0", dict(max_seg=0), BAD_ARG),
                 (fn, "NULL long_ws", dict(long_ws=None), BAD_ARG)]
    rows += [("gsl_fused_absgrad", what, over, BAD_ARG) for what, over in _GEOMETRY
             if not any(k in over for k in ("ty0", "row0"))]
    for fn in ("gsl_fused_raster_fwd", "gsl_long_raster_fwd", "gsl_fused_raster_bwd", "gsl_long_raster_bwd",
               "gsl_tiny_raster_bwd", "gsl_fused_absgrad"):
        rows += [(fn, "NULL tile_offsets", dict(tile_offsets=None), BAD_ARG),
                 (fn, "NULL alphas", dict(alphas=None), BAD_ARG),
                 (fn, "ed with three channels", dict(channels=3, ed=1), BAD_ARG),
                 (fn, "early OK: the base call", {}, OK)]
    rows += [
        ("gsl_fused_raster_fwd", "hit list without its lengths", dict(isect_hit_counts=None), BAD_ARG),
        ("gsl_fused_raster_fwd", "sorting forward on a strip", dict(sort_bins=0x1000, bin_cap=64, ty0=1, ty1=1), BAD_ARG),
        ("gsl_fused_raster_bwd", "early OK: capacity == 0", dict(capacity=0, ty1=3), OK),
        ("gsl_fused_raster_bwd", "early OK: row0 == row1", dict(row0=16, row1=16, ty1=3), OK),
        ("gsl_fused_raster_bwd", "NULL flatten_ids", dict(flatten_ids=None, ty1=3), BAD_ARG),
        ("gsl_fused_raster_bwd", "neither vacc nor vrow", dict(vacc=None, vrow=None, ty1=3), BAD_ARG),
        ("gsl_fused_raster_bwd", "vrow with clear_ws", dict(vrow=0x1000, clear_ws=0x1000, ty1=3), BAD_ARG),
        ("gsl_long_raster_bwd", "early OK: capacity == 0", dict(capacity=0, ty1=3), OK),
        ("gsl_long_raster_bwd", "early OK: row0 == row1", dict(row0=16, row1=16, ty1=3), OK),
        ("gsl_long_raster_bwd", "NULL vacc", dict(vacc=None), BAD_ARG),
        ("gsl_long_raster_bwd", "NULL flatten_ids", dict(flatten_ids=None, ty1=3), BAD_ARG),
        ("gsl_long_raster_fwd", "early OK: capacity == 0", dict(capacity=0, ty1=3), OK),
        ("gsl_long_raster_fwd", "short workspace alone", dict(long_ws_bytes=0), WORKSPACE),
        ("gsl_long_raster_fwd", "short workspace + ed with three channels", dict(long_ws_bytes=0, channels=3), WORKSPACE),
        ("gsl_long_raster_fwd", "short workspace + NULL flatten_ids", dict(long_ws_bytes=0, flatten_ids=None), WORKSPACE),
        ("gsl_long_raster_fwd", "short workspace + NULL tile_offsets", dict(long_ws_bytes=0, tile_offsets=None), BAD_ARG),
        ("gsl_long_raster_fwd", "short workspace + max_seg <= 0", dict(long_ws_bytes=0, max_seg=0), BAD_ARG),
        ("gsl_tiny_raster_bwd", "NULL trec", dict(trec=None), BAD_ARG),
        ("gsl_tiny_raster_bwd", "fused loss on a strip", dict(loss_depth_gt=0x1000), BAD_ARG),
        ("gsl_tiny_raster_bwd", "fused loss with three channels",
         dict(loss_depth_gt=0x1000, ty1=3, channels=3, ed=0, Q0=None), BAD_ARG),
        ("gsl_fused_absgrad", "two channels", dict(channels=2, ed=0), BAD_ARG),
        ("gsl_fused_absgrad", "ed without render", dict(render=None), BAD_ARG),
        ("gsl_fused_absgrad", "hit list without its lengths", dict(isect_hit_counts=None), BAD_ARG),
        ("gsl_fused_absgrad", "NULL records with entries", dict(capacity=100, Q0=None), BAD_ARG),
    ]
    fn = "gsl_fused_project"
    rows += [(fn, what, over, BAD_ARG) for what, over in _GEOMETRY if not any(k in over for k in ("capacity", "row0"))
             and what not in ("ty0 < 0", "ty1 > tile_h")]
    rows += [
        (fn, "ty0 < 0", dict(ty0=-1), BAD_ARG), (fn, "ty1 > tile_h", dict(ty1=4), BAD_ARG),
        (fn, "N < 0", dict(N=-1), BAD_ARG), (fn, "N > 2^26", dict(N=(1 << 26) + 1), BAD_ARG),
        (fn, "NULL viewmat", dict(viewmat=None), BAD_ARG), (fn, "NULL n_isects", dict(n_isects=None), BAD_ARG),
        (fn, "colour records without colours", dict(colors=None), BAD_ARG),
        (fn, "SH degree above 3", dict(sh_degree=4, K_sh=25), BAD_ARG),
        (fn, "anti-aliasing without compensations", dict(antialiased=1, compensations=None), BAD_ARG),
        (fn, "early OK: N == 0, binned", {}, OK),
        (fn, "short workspace alone", dict(ws_bytes=0), WORKSPACE), (fn, "NULL workspace", dict(ws=None), WORKSPACE),
        (fn, "short workspace + bins without capacity", dict(ws_bytes=0, bin_cap=0), WORKSPACE),
        (fn, "short workspace + NULL viewmat", dict(ws_bytes=0, viewmat=None), BAD_ARG),
        (fn, "short workspace + N < 0", dict(ws_bytes=0, N=-1), BAD_ARG),
        (fn, "bins without capacity", dict(bin_cap=0), BAD_ARG),
    ]
    fn, binned = "gsl_fused_bin", dict(bins=0x1000, bin_cap=64, capacity=100, ws_bytes=0)
    rows += [
        (fn, "N < 0", dict(N=-1), BAD_ARG), (fn, "tile_w <= 0", dict(tile_w=0), BAD_ARG),
        (fn, "tile_h <= 0", dict(tile_h=0), BAD_ARG), (fn, "ty0 < 0", dict(ty0=-1), BAD_ARG),
        (fn, "ty1 > tile_h", dict(ty1=4), BAD_ARG), (fn, "ty0 > ty1", dict(ty0=2, ty1=1), BAD_ARG),
        (fn, "capacity < 0", dict(capacity=-1), BAD_ARG), (fn, "NULL tile_offsets", dict(tile_offsets=None), BAD_ARG),
        (fn, "early OK: N == 0", dict(capacity=100), OK), (fn, "early OK: capacity == 0", dict(N=256), OK),
        (fn, "early OK: empty strip", dict(N=256, capacity=100, ty0=1, ty1=1), OK),
        (fn, "early OK comes before the pointers", dict(Q0=None, sort_keys=None, ws=None), OK),
        (fn, "binned, short workspace alone", binned, WORKSPACE),
        (fn, "binned, short workspace + NULL sort_keys", dict(binned, sort_keys=None), WORKSPACE),
        (fn, "binned, short workspace + bins without capacity", dict(binned, bin_cap=0), BAD_ARG),
        (fn, "binned, short workspace + NULL n_isects", dict(binned, n_isects=None), BAD_ARG),
    ]
    fn = "gsl_fused_project_bwd"
    rows += [
        (fn, "N < 0", dict(N=-1), BAD_ARG), (fn, "width <= 0", dict(width=0), BAD_ARG),
        (fn, "height <= 0", dict(height=0), BAD_ARG), (fn, "n_tiles <= 0", dict(n_tiles=0), BAD_ARG),
        (fn, "two channels", dict(channels=2), BAD_ARG),
        (fn, "NULL v_quats beside v_means", dict(v_quats=None), BAD_ARG),
        (fn, "full gradients without v_colors", dict(v_colors=None), BAD_ARG),
        (fn, "anti-aliasing without compensations", dict(antialiased=1, compensations=None), BAD_ARG),
        (fn, "early OK: N == 0", {}, OK), (fn, "early OK comes before the workspace", dict(ws_bytes=0, means=None), OK),
        (fn, "short workspace alone", _SHORT_WS, WORKSPACE),
        (fn, "short workspace + NULL means", dict(_SHORT_WS, means=None), BAD_ARG),
        (fn, "short workspace + no gradient rows", dict(_SHORT_WS, vacc=None), BAD_ARG),
        (fn, "short workspace + NULL colors", dict(_SHORT_WS, colors=None), BAD_ARG),
        (fn, "short workspace + rows of another grid", dict(_SHORT_WS, vrow=0x1000, n_tiles=13), BAD_ARG),
    ]
    return rows


ROWS = _rows()


def _guarded(fn, over):
    """True if the call still carries an early-return guard of its entry point (whatever else it violates)."""
    a = dict(BASE[fn], **over)
    if fn == "gsl_fused_absgrad":
        return a["capacity"] == 0
    if fn == "gsl_fused_project":
        return a["N"] <= 0 and "bins" not in over
    if fn == "gsl_fused_bin":
        return a["bins"] is None and (a["N"] <= 0 or a["capacity"] <= 0 or a["ty0"] >= a["ty1"])
    if fn == "gsl_fused_project_bwd":
        return a["N"] <= 0 and a["reduce_viewmat"] == 0
    guard = a["ty0"] >= a["ty1"]
    if fn in ("gsl_fused_raster_bwd", "gsl_long_raster_bwd"):
        guard = guard or a["capacity"] <= 0 or a["row0"] >= a["row1"]
    if fn == "gsl_long_raster_fwd":
        guard = guard or a["capacity"] <= 0
    return guard


def call(lib, params, fn, over, dummy):
    """Call fn (parameters as the header lists them) with BASE[fn] updated by over; every pointer that is not named
    gets the dummy host buffer."""
    named = dict(BASE[fn], **over)
    assert set(named) <= {n for _, n in params}, (fn, sorted(set(named) - {n for _, n in params}))
    n_tiles = named.get("n_tiles", named.get("tile_w", 0) * named.get("tile_h", 0))
    full = {"ws_bytes": lambda: lib.gsl_fused_ws_bytes(max(named.get("N", 0), 0), n_tiles),
            "long_ws_bytes": lambda: lib.gsl_long_ws_bytes(named.get("max_seg", 0))}
    args = []
    for c_type, name in params:
        if name == "stream":
            args.append(None)
        elif name in named:
            args.append(full[name]() if named[name] == _FULL else named[name])
        else:
            args.append(dummy if "*" in c_type else 0)
    return getattr(lib, fn)(*args)


def test_the_table_covers_every_entry_point_and_case_class():
    for fn in BASE:
        what = [w for f, w, _, _ in ROWS if f == fn]
        assert len(what) == len(set(what)), fn
        assert any(w.startswith("early OK") for w in what) and any(w.startswith("NULL") for w in what), fn
        if "ed" in BASE[fn]:
            assert "ed with three channels" in what, fn
    for fn in ("gsl_long_raster_fwd", "gsl_fused_project", "gsl_fused_bin", "gsl_fused_project_bwd"):
        both = {e for f, w, _, e in ROWS if f == fn and "short workspace" in w}
        assert both == {BAD_ARG, WORKSPACE}, fn  # the order of the two statuses is pinned from both sides


@pytest.mark.parametrize("fn", sorted(BASE))
def test_status_of_calls_that_return_before_any_launch(fn, repo_root):
    lib = _lib.load_library()
    params = prototypes(repo_root)[fn][1]
    buf = ctypes.create_string_buffer(256)
    dummy = ctypes.addressof(buf)
    for f, what, over, expected in ROWS:
        if f != fn:
            continue
        # no row may reach a launch: it keeps a guard, or it is refused -- and GSL_ERR_HIP is what a launch would give here
        assert expected in (OK, BAD_ARG, WORKSPACE) and (_guarded(fn, over) or expected != OK), (fn, what)
        got = call(lib, params, fn, over, dummy)
        assert got != ERR_HIP, (fn, what)
        assert got == expected, (fn, what, got, expected)
