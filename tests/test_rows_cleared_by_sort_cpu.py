"""Host side of "the sort launch clears the gradient rows" (no GPU needed): the argument checks of the new entry points
gsl_fused_bin_clear / gsl_fused_project_bwd_keep / gsl_fused_clear_rows, their Python callers against the header, and
the state RenderContext keeps about who owes the clearing (_sort_cleared, _rows_dirty), with the launches stubbed out.

The status table has the form of tests/test_entry_checks_cpu.py: no row may reach a launch (the pointers are dummy HOST
buffers), so every row keeps an early-return guard or fails a check in front of the first launch.  gsl_fused_bin_clear
with N > 0 has no early return without a launch -- the rows are zeroed whichever way the call ends -- so its guarded
rows have N = 0.
"""
import ctypes

import pytest
import torch

import tests.test_entry_checks_cpu as EC
import tests.test_stages_cpu as SC
from gsplatloc_amd import _lib
from tests.test_abi import prototypes

OK, BAD_ARG, WORKSPACE, ERR_HIP = 0, -1, -2, -3
_FULL = "full"
PAIRS = {"gsl_fused_bin_clear": "gsl_fused_bin", "gsl_fused_project_bwd_keep": "gsl_fused_project_bwd"}

BASE = {
    "gsl_fused_bin_clear": dict(EC.BASE["gsl_fused_bin"]),
    "gsl_fused_project_bwd_keep": dict(EC.BASE["gsl_fused_project_bwd"]),
    "gsl_fused_clear_rows": dict(N=0),
}
_BINNED = dict(bins=0x1000, bin_cap=64, capacity=100, ws_bytes=0)
_SHORT_WS = dict(N=256, reduce_viewmat=0, ws_bytes=0)
ROWS = [
    # the additions: a row buffer with N > 0 must not be NULL, N < 0 is a bad argument
    ("gsl_fused_bin_clear", "N < 0", dict(N=-1), BAD_ARG),
    ("gsl_fused_bin_clear", "NULL rows with N > 0", dict(N=256, rows=None), BAD_ARG),
    ("gsl_fused_bin_clear", "NULL rows with N > 0, binned, short workspace", dict(_BINNED, N=256, rows=None), BAD_ARG),
    ("gsl_fused_bin_clear", "N > 2^26", dict(N=(1 << 26) + 1), BAD_ARG),
    ("gsl_fused_bin_clear", "early OK: N == 0, NULL rows", dict(rows=None, capacity=100), OK),
    ("gsl_fused_bin_clear", "early OK: N == 0", dict(capacity=100), OK),
    ("gsl_fused_bin_clear", "binned, short workspace alone", _BINNED, WORKSPACE),
    ("gsl_fused_bin_clear", "binned, short workspace + bins without capacity", dict(_BINNED, bin_cap=0), BAD_ARG),
    ("gsl_fused_project_bwd_keep", "N < 0", dict(N=-1), BAD_ARG),
    ("gsl_fused_project_bwd_keep", "NULL vacc with N > 0", dict(_SHORT_WS, vacc=None), BAD_ARG),
    ("gsl_fused_project_bwd_keep", "deterministic rows", dict(vrow=0x1000), BAD_ARG),
    ("gsl_fused_project_bwd_keep", "tiny-splat slabs", dict(tiny_trec=0x1000), BAD_ARG),
    ("gsl_fused_project_bwd_keep", "early OK: N == 0", {}, OK),
    ("gsl_fused_project_bwd_keep", "short workspace alone", _SHORT_WS, WORKSPACE),
    ("gsl_fused_project_bwd_keep", "short workspace + NULL means", dict(_SHORT_WS, means=None), BAD_ARG),
    ("gsl_fused_clear_rows", "N < 0", dict(N=-1), BAD_ARG),
    ("gsl_fused_clear_rows", "NULL rows with N > 0", dict(N=256, rows=None), BAD_ARG),
    ("gsl_fused_clear_rows", "early OK: N == 0", {}, OK),
    ("gsl_fused_clear_rows", "early OK: N == 0, NULL rows", dict(rows=None), OK),
]


def _call(lib, fn, params, named, dummy):
    assert set(named) <= {n for _, n in params}, (fn, sorted(set(named) - {n for _, n in params}))
    n_tiles = named.get("n_tiles", named.get("tile_w", 0) * named.get("tile_h", 0))
    args = []
    for c_type, name in params:
        if name == "stream":
            args.append(None)
        elif name in named:
            v = named[name]
            args.append(lib.gsl_fused_ws_bytes(max(named.get("N", 0), 0), n_tiles) if v == _FULL else v)
        else:
            args.append(dummy if "*" in c_type else 0)
    return getattr(lib, fn)(*args)


def _reaches_a_launch(fn, named):
    """Would a call that passes every check launch something?  (Then it may not be in a table of host pointers.)"""
    if fn == "gsl_fused_project_bwd_keep":
        return named["N"] > 0 or named["reduce_viewmat"] != 0
    return named["N"] > 0


@pytest.mark.parametrize("fn", sorted(BASE))
def test_status_of_calls_that_return_before_any_launch(fn, repo_root):
    lib = _lib.load_library()
    params = prototypes(repo_root)[fn][1]
    buf = ctypes.create_string_buffer(256)
    dummy = ctypes.addressof(buf)
    rows = [r for r in ROWS if r[0] == fn]
    assert any(e == OK for *_, e in rows) and any(e == BAD_ARG for *_, e in rows)
    for _, what, over, expected in rows:
        named = dict(BASE[fn], **over)
        assert expected != OK or not _reaches_a_launch(fn, named), (fn, what)
        got = _call(lib, fn, params, named, dummy)
        assert got != ERR_HIP, (fn, what)
        assert got == expected, (fn, what, got, expected)


@pytest.mark.parametrize("fn", sorted(PAIRS))
def test_the_new_entry_points_share_the_ladder_of_the_old(fn, repo_root):
    """Every row of the pinned table of the old entry point gives the same status through the new one (its row buffer
    a dummy) -- less the rows that end GSL_OK with N > 0: there the new entry point has rows to zero and launches."""
    lib = _lib.load_library()
    old = PAIRS[fn]
    protos = prototypes(repo_root)
    assert [p for p in protos[fn][1] if p[1] != "rows"] == protos[old][1]
    buf = ctypes.create_string_buffer(256)
    dummy = ctypes.addressof(buf)
    n = 0
    for f, what, over, expected in EC.ROWS:
        named = dict(EC.BASE[old], **over)
        if f != old or (expected == OK and _reaches_a_launch(fn, named)):
            continue
        if fn == "gsl_fused_project_bwd_keep" and (named.get("vrow") or named.get("tiny_trec")):
            expected = BAD_ARG
        assert _call(lib, fn, protos[fn][1], named, dummy) == expected, (fn, what)
        n += 1
    assert n >= 12, n


@pytest.mark.parametrize("caller", ["fused_bin_clear", "fused_project_bwd_keep"])
def test_caller_passes_the_headers_argument_list(caller, repo_root, monkeypatch):
    SC.test_caller_passes_the_headers_argument_list(caller, repo_root, monkeypatch)


def test_clear_rows_caller(monkeypatch):
    import types

    from gsplatloc_amd import stages

    got, stream = [], object()
    monkeypatch.setattr(stages, "load_library", lambda: types.SimpleNamespace(gsl_fused_clear_rows=lambda *a: got.append(a) or 0))
    monkeypatch.setattr(stages, "current_stream", lambda: stream)
    stages.fused_clear_rows(torch.zeros(3, 16), 3)
    assert len(got) == 1 and got[0][1:] == (3, stream) and got[0][0] != 0


# ------------------------------------------------------------------------------------------------ RenderContext
def _context(**kw):
    import gsplatloc_amd.context as CX
    from gsplatloc_amd.synthetic import perturbed_pose, random_scene

    N, W, H = 500, 64, 48
    ctx = CX.RenderContext(N, W, H, "RGB+ED", sh_degree=1, K_sh=4, device="cpu", **kw)
    ctx._alloc_isects(4096)
    sc = random_scene(N, W, H, sigma_px=1.0)
    inp = (sc["means"], sc["quats"], sc["scales"], sc["opacities"], sc["sh"],
           torch.linalg.inv(perturbed_pose()).contiguous(), sc["K"].contiguous())
    return ctx, inp, torch.zeros(H, W, ctx.D), torch.zeros(H, W, 1)


@pytest.mark.skipif(torch.cuda.is_available(), reason="host-pointer calls: only meaningful without a GPU")
def test_render_context_reaches_the_new_calls(monkeypatch):
    """Refused by the HIP runtime (-3), which only happens once ctypes has accepted the argument list and the entry
    point's own checks have passed."""
    import gsplatloc_amd.stages as ST

    monkeypatch.setattr(ST, "current_stream", lambda: None)
    ctx, inp, v, va = _context()
    ctx._inputs = inp
    assert ctx.sort_clears_rows()
    with pytest.raises(RuntimeError, match=r"gsl_fused_bin_clear failed: HIP launch error \(status -3\)"):
        ctx._bin()
    assert not ctx._sort_cleared and not ctx._rows_dirty
    ctx._sort_cleared = True  # as a sort launch that ran would have left it
    with pytest.raises(RuntimeError, match=r"gsl_fused_project_bwd_keep failed: HIP launch error \(status -3\)"):
        ctx._project_bwd(True)
    assert ctx._rows_dirty
    with pytest.raises(RuntimeError, match=r"gsl_fused_clear_rows failed: HIP launch error \(status -3\)"):
        ctx._raster_bwd(v, va)
    assert ctx._rows_dirty  # (the refused call has cleared nothing)


STAGES = ["fused_project", "fused_bin", "fused_bin_clear", "fused_clear_rows", "fused_raster_fwd", "fused_raster_bwd",
          "tiny_raster_bwd", "long_sort", "long_raster_fwd", "long_raster_bwd", "fused_project_bwd", "fused_project_bwd_keep"]
ROW_CALLS = ("fused_bin", "fused_bin_clear", "fused_clear_rows", "fused_raster_bwd", "tiny_raster_bwd", "fused_project_bwd",
             "fused_project_bwd_keep")


def _stubbed(monkeypatch, **kw):
    import gsplatloc_amd.stages as ST

    calls, fail = [], set()

    def stub(name):
        def f(*a, **k):
            if name in fail:
                raise RuntimeError(f"gsl_{name} failed: HIP launch error (status -3)")
            calls.append(name)
        return f

    for name in STAGES:
        monkeypatch.setattr(ST, name, stub(name))
    ctx, inp, v, va = _context(**kw)

    def run(ops):
        del calls[:]
        for op in ops.split():
            ctx.forward(*inp) if op == "F" else ctx.backward(v, va, full=True)
        return [c for c in calls if c in ROW_CALLS]

    return ctx, run, fail, inp


NEW_F, NEW_B = ["fused_bin_clear"], ["fused_raster_bwd", "fused_project_bwd_keep"]
OLD_F, OLD_B = ["fused_bin"], ["fused_raster_bwd", "fused_project_bwd"]


def test_state_steady_and_repeated_calls(monkeypatch):
    ctx, run, _, _ = _stubbed(monkeypatch)
    assert run("F B F B F B") == (NEW_F + NEW_B) * 3  # steady state: nobody but the sort clears
    assert ctx._rows_dirty and ctx._sort_cleared
    assert run("F F B") == NEW_F * 2 + NEW_B
    # a second backward after one forward finds the rows standing and clears them itself, before the compositing launch
    assert run("F B B B") == NEW_F + NEW_B + (["fused_clear_rows"] + NEW_B) * 2
    assert ctx._rows_dirty
    assert run("F") == NEW_F and not ctx._rows_dirty


def test_state_switch_read_per_call(monkeypatch):
    ctx, run, _, _ = _stubbed(monkeypatch)
    monkeypatch.setenv("GSLOC_SORT_CLEARS_ROWS", "0")
    assert not ctx.sort_clears_rows()
    assert run("F B F B B") == OLD_F + OLD_B + OLD_F + OLD_B * 2 and not ctx._rows_dirty
    monkeypatch.setenv("GSLOC_SORT_CLEARS_ROWS", "1")
    assert run("F B") == NEW_F + NEW_B and ctx._rows_dirty
    # switched off between a backward that kept the rows and the next forward: its sort clears nothing, so the backward does
    monkeypatch.setenv("GSLOC_SORT_CLEARS_ROWS", "0")
    assert run("F B F B") == OLD_F + ["fused_clear_rows"] + OLD_B + OLD_F + OLD_B
    assert not ctx._rows_dirty and not ctx._sort_cleared
    # switched on between a forward and its backward: that forward's sort has not cleared, so this backward still does
    assert run("F") == OLD_F
    monkeypatch.setenv("GSLOC_SORT_CLEARS_ROWS", "1")
    assert run("B") == OLD_B and not ctx._rows_dirty


def test_state_after_a_failed_sort(monkeypatch):
    ctx, run, fail, _ = _stubbed(monkeypatch)
    assert run("F B") == NEW_F + NEW_B and ctx._rows_dirty
    fail.add("fused_bin_clear")
    with pytest.raises(RuntimeError, match="gsl_fused_bin_clear failed"):
        run("F")
    assert ctx._rows_dirty and not ctx._sort_cleared  # a refused or failed sort call has cleared nothing
    fail.clear()
    # (a caller that goes on regardless: the backward clears the rows and, its forward's sort not having cleared, again)
    assert run("B") == ["fused_clear_rows"] + OLD_B and not ctx._rows_dirty
    assert run("F B") == NEW_F + NEW_B


def test_contexts_that_keep_the_earlier_contract(monkeypatch):
    for kw, tiny in ((dict(deterministic=True), False), (dict(sort_in_forward=True), True), ({}, True)):
        ctx, run, _, _ = _stubbed(monkeypatch, **kw)
        if kw.get("deterministic"):
            ctx._alloc_isects(4096)
        if tiny:
            ctx.tiny, ctx.trec, ctx.vcT = True, torch.zeros(ctx.N, 32), torch.zeros(ctx.H, ctx.W, ctx.D)
        if kw.get("sort_in_forward"):
            ctx.bins, ctx.bin_cap = torch.zeros(ctx.n_tiles * 64, dtype=torch.int64), 64
            assert ctx.sorts_in_forward()
        assert not ctx.sort_clears_rows()
        got = run("F B F B B")
        assert not any(c in got for c in ("fused_bin_clear", "fused_clear_rows", "fused_project_bwd_keep")), (kw, got)
        assert got.count("fused_project_bwd") == 3 and not ctx._rows_dirty and not ctx._sort_cleared


def test_calibrate_leaves_a_consistent_state(monkeypatch):
    """calibrate() between a backward that left the rows standing and the next step -- here it even changes the kind of
    backward (nothing was projected, so every r_cull is 0 and it picks the tiny-splat one): whoever runs next finds the
    debt recorded and pays it before a compositing launch can add into the rows."""
    ctx, run, _, inp = _stubbed(monkeypatch)
    assert run("F B") == NEW_F + NEW_B and ctx._rows_dirty
    ctx.calibrate(*inp)
    assert ctx._rows_dirty
    if ctx.tiny:
        assert not ctx.sort_clears_rows()
        assert run("F B F B") == OLD_F + ["fused_clear_rows", "tiny_raster_bwd", "fused_project_bwd"] + OLD_F + [
            "tiny_raster_bwd", "fused_project_bwd"]
    else:
        assert run("F B F B") == (NEW_F + NEW_B) * 2
    ctx.use_general_backward()
    assert run("F B B") == NEW_F + NEW_B + ["fused_clear_rows"] + NEW_B
