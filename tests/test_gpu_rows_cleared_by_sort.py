"""The gradient rows cleared by the sort launch of the next forward instead of by the projection backward.

The compositing backward adds into RenderContext.vacc and must find it zero.  A context with the general,
non-deterministic backward and a sort launch of its own has that launch clear the rows (gsl_fused_bin_clear) and its
projection backward leave them standing (gsl_fused_project_bwd_keep); GSLOC_SORT_CLEARS_ROWS=0 is the earlier
behaviour, where the projection backward clears what it read.  What can go wrong: a row the sort does not clear (its
gradient is then the sum of two steps: an error of order 1), a store past the rows, a sequence of calls after which
nobody has cleared them, and a context that must keep the earlier contract but does not.

"Same gradients" below: within 1e-3 of the largest magnitude of each tensor.  A condition, not a measurement: an
uncleared row doubles a gradient, two orders of float atomics differ by about 1e-6 at these sizes.
"""
import contextlib
import functools
import os

import pytest
import torch

from gsplatloc_amd import stages
from gsplatloc_amd.context import RenderContext
from tests.scenes import random_scene, sh_from_rgb, small_pose
from tests.sort_variants import forced_tile_sort

pytestmark = pytest.mark.gpu
DEV = "cuda"
SWITCH = "GSLOC_SORT_CLEARS_ROWS"
N = 4099
FRAMES = {"6x4 tiles": (96, 64), "5x3 tiles": (80, 48)}  # the last workgroup of the wave sorts full / partly empty
BOUND = 1e-3
NEW = ("fused_bin_clear", "fused_project_bwd_keep", "fused_clear_rows")
OLD = ("fused_bin", "fused_project_bwd")


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def _inputs(n, W, H):
    # (anisotropic: the quaternion gradient of an isotropic Gaussian is zero in exact arithmetic, and a tensor of rounding
    # residue cannot be compared relative to its own largest entry)
    sc = random_scene(n, W, H, dtype=torch.float32, sigma_px=1.0, aniso=True)
    V = torch.linalg.inv(small_pose(0.5, 0.01, dtype=torch.float32)).contiguous()
    ins = tuple(t.to(DEV).contiguous() for t in (sc["means"], sc["quats"], sc["scales"], sc["opacities"],
                                                 sh_from_rgb(sc["rgbs"]), V, sc["K"]))
    g = torch.Generator().manual_seed(11)
    v = torch.randn(H, W, 4, generator=g).to(DEV)
    va = torch.randn(H, W, 1, generator=g).to(DEV)
    return ins, v, va


def _context(n, W, H, **kw):
    ins, _, _ = _inputs(n, W, H)
    rc = RenderContext(n, W, H, "RGB+ED", sh_degree=1, K_sh=4, device=DEV, **kw)
    rc.calibrate(*ins)
    return rc


def _step(rc, n, W, H, forward=True):
    ins, v, va = _inputs(n, W, H)
    if forward:
        rc.forward(*ins)
    g = rc.grads_in_input_order(rc.backward(v, va, full=True))
    torch.cuda.synchronize()
    return {k: t.clone() for k, t in g.items() if t is not None}


@functools.lru_cache(maxsize=None)
def _reference(n, W, H, tile_rows=None):
    """The first backward of a fresh context with the switch off; computed once, never written to."""
    with _env(**{SWITCH: "0"}):
        rc = _context(n, W, H, tile_rows=tile_rows)
        assert not rc.sort_clears_rows() and not rc.tiny
        return _step(rc, n, W, H)


def _assert_same(got, want, what):
    assert set(got) == set(want) and {"viewmat", "means", "quats", "scales", "opacities", "colors"} <= set(got)
    for k in want:
        assert bool(torch.isfinite(got[k]).all()), (what, k, "not finite")
        top = float(want[k].abs().max())
        assert top > 0, (what, k)
        err = float((got[k] - want[k]).abs().max())
        assert err <= BOUND * top, (what, k, err, top)


def _spy(monkeypatch):
    calls = []
    for name in NEW + OLD:
        real = getattr(stages, name)
        monkeypatch.setattr(stages, name, lambda *a, _real=real, _name=name, **k: (calls.append(_name), _real(*a, **k))[1])
    return calls


def _poisoned_step(monkeypatch, kernel, n, W, H, **kw):
    rc = _context(n, W, H, **kw)
    assert rc.sort_clears_rows() and not rc.tiny and not rc.deterministic
    rc.vacc.fill_(float("nan"))
    calls = _spy(monkeypatch)
    with forced_tile_sort(monkeypatch, kernel):
        got = _step(rc, n, W, H)
    assert calls == ["fused_bin_clear", "fused_project_bwd_keep"], calls
    return rc, got


@pytest.mark.parametrize("kernel", ["wave16", "wave32", "wg"])
@pytest.mark.parametrize("frame", sorted(FRAMES) + ["one tile"])
def test_sort_clears_every_poisoned_row(frame, kernel, monkeypatch):
    """Rows full of NaN before the forward: one row the sort launch leaves is a NaN in a gradient."""
    n, (W, H) = (2000, (16, 16)) if frame == "one tile" else (N, FRAMES[frame])
    rc, got = _poisoned_step(monkeypatch, kernel, n, W, H)
    assert rc.bins is not None  # (the binned path: the sort launch runs over all tiles)
    _assert_same(got, _reference(n, W, H), (frame, kernel))


@pytest.mark.parametrize("kernel", ["wave16", "wg"])
def test_sort_clears_every_poisoned_row_two_pass_and_strip(kernel, monkeypatch):
    W, H = FRAMES["6x4 tiles"]
    with _env(GSLOC_BINNING="two-pass"):
        rc, got = _poisoned_step(monkeypatch, kernel, N, W, H)
    assert rc.bins is None
    _assert_same(got, _reference(N, W, H), ("two-pass", kernel))
    for binning in ("direct", "two-pass"):  # a strip: the binned launch runs over all tiles, the two-pass one over the strip's
        with _env(GSLOC_BINNING=binning):
            rc, got = _poisoned_step(monkeypatch, kernel, N, W, H, tile_rows=(1, 3))
        assert (rc.bins is None) == (binning == "two-pass")
        _assert_same(got, _reference(N, W, H, (1, 3)), ("strip", binning, kernel))


@pytest.mark.parametrize("kernel", ["wave16", "wave32", "wg"])
@pytest.mark.parametrize("frame", sorted(FRAMES) + ["one tile"])
def test_rows_past_the_length_are_not_touched(frame, kernel, monkeypatch):
    """The stage handed a buffer of N + 64 rows and the length N: rows 0 .. N-1 zero, the tail as it was."""
    n, (W, H) = (2000, (16, 16)) if frame == "one tile" else (N, FRAMES[frame])
    ins, _, _ = _inputs(n, W, H)
    rc = _context(n, W, H)
    rows = torch.full((n + 64, 16), 7.25, device=DEV)
    rc._project(*ins)
    with forced_tile_sort(monkeypatch, kernel):
        stages.fused_bin_clear(rc.Q0, rc.radii, n, rc.tw, rc.th, rc.ty0, rc.ty1, stages.tile_n_bits(rc.n_tiles), rc.offs,
                               rc.capacity, rc.keys, rc.flatten_ids, rc.ws, rows, bins=rc.bins, bin_cap=rc.bin_cap,
                               n_isects=rc.n_is, flags=rc.flags, long_min=rc.long_min if rc.bins is not None else 0)
        torch.cuda.synchronize()
    assert int((rows[:n] != 0).sum()) == 0
    assert bool((rows[n:] == 7.25).all())
    rc._raster_fwd()  # (leaves the tile counters as the next projection expects them)


def test_rows_are_cleared_where_no_sort_launches():
    """capacity 0 / an empty strip: gsl_fused_bin returns without a sort launch, the rows are zeroed all the same."""
    W, H = FRAMES["6x4 tiles"]
    rc = _context(N, W, H)
    for ty0, ty1, capacity in ((0, rc.th, 0), (2, 2, rc.capacity)):
        rows = torch.full((N + 64, 16), 7.25, device=DEV)
        stages.fused_bin_clear(rc.Q0, rc.radii, N, rc.tw, rc.th, ty0, ty1, stages.tile_n_bits(rc.n_tiles), rc.offs,
                               capacity, rc.keys, rc.flatten_ids, rc.ws, rows)
        torch.cuda.synchronize()
        assert int((rows[:N] != 0).sum()) == 0 and bool((rows[N:] == 7.25).all()), (ty0, ty1, capacity)


@pytest.mark.parametrize("sequence", ["FB FB FB", "F F B", "F B B", "F B calibrate F B"])
def test_every_backward_of_a_sequence_matches_a_fresh_context(sequence):
    W, H = FRAMES["5x3 tiles"]
    want = _reference(N, W, H)
    rc = _context(N, W, H)
    assert rc.sort_clears_rows()
    ins, v, va = _inputs(N, W, H)
    n_bwd = 0
    for op in sequence.replace("FB", "F B").split():
        if op == "F":
            rc.forward(*ins)
            assert not rc._rows_dirty
        elif op == "calibrate":
            rc.calibrate(*ins)
        else:
            n_bwd += 1
            _assert_same(_step(rc, N, W, H, forward=False), want, (sequence, n_bwd))
            assert rc._rows_dirty
    assert n_bwd >= 1


def test_a_captured_step_replays_like_the_eager_one():
    """Forward + backward in one HIP graph, as the benchmark runs them: the sort launch of each replay clears what the
    projection backward of the replay before left standing."""
    W, H = FRAMES["6x4 tiles"]
    rc = _context(N, W, H)
    assert rc.sort_clears_rows()
    ins, v, va = _inputs(N, W, H)
    eager = _step(rc, N, W, H)
    _assert_same(eager, _reference(N, W, H), "eager")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        rc.forward(*ins)
        rc.backward(v, va, full=True)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            rc.forward(*ins)
            out = rc.backward(v, va, full=True)
    torch.cuda.synchronize()
    for replay in range(3):
        graph.replay()
        torch.cuda.synchronize()
        got = {k: t.clone() for k, t in rc.grads_in_input_order(out).items() if t is not None}
        _assert_same(got, eager, ("replay", replay))


def _depth_frame(W, H, pile):
    from gsplatloc_amd.synthetic import depth_frame_scene

    sc = depth_frame_scene(W, H, stride=1, holes=pile, device=DEV, pile=pile)
    # (made anisotropic, for the reason given at _inputs; the axes only shrink, so the splats stay tiny)
    g = torch.Generator().manual_seed(5)
    quats = torch.randn(sc["N"], 4, generator=g).to(DEV)
    scales = (sc["scales"] * (0.5 + 0.5 * torch.rand(sc["N"], 3, generator=g).to(DEV))).contiguous()
    return (sc["means"], quats, scales, sc["opacities"], sc["sh"], sc["viewmat"], sc["K"].contiguous()), sc["N"]


@pytest.mark.parametrize("kind", ["tiny", "sort in forward", "deterministic", "long list", "switch off"])
def test_contexts_that_keep_the_earlier_contract(kind, monkeypatch):
    """Tiny-splat contexts, the sorting forward, the deterministic mode, a frame with a long list (tiny-splat backward +
    gsl_long_raster_bwd adding into the rows) and the switch at 0: the projection backward clears what it read, through
    the entry points that were there before -- and repeated steps give the first step's gradients."""
    if kind == "switch off":
        monkeypatch.setenv(SWITCH, "0")
    if kind in ("tiny", "sort in forward", "long list"):
        W, H = (320, 240) if kind == "long list" else (160, 120)
        ins, n = _depth_frame(W, H, pile=kind == "long list")
        rc = RenderContext(n, W, H, "RGB+ED", sh_degree=1, K_sh=4, device=DEV, sort_in_forward=kind == "sort in forward")
        rc.calibrate(*ins)
        assert rc.tiny and rc.sorts_in_forward() == (kind == "sort in forward")
        assert (rc.long_min > 0) == (kind == "long list")
    else:
        W, H = FRAMES["6x4 tiles"]
        n = N
        ins, _, _ = _inputs(n, W, H)
        rc = _context(n, W, H, deterministic=kind == "deterministic")
        assert not rc.tiny
    assert not rc.sort_clears_rows()
    g = torch.Generator().manual_seed(11)
    v, va = torch.randn(H, W, 4, generator=g).to(DEV), torch.randn(H, W, 1, generator=g).to(DEV)
    calls = _spy(monkeypatch)
    steps = []
    for _ in range(3):
        rc.forward(*ins)
        out = rc.grads_in_input_order(rc.backward(v, va, full=True))
        torch.cuda.synchronize()
        steps.append({k: t.clone() for k, t in out.items() if t is not None})
        assert not rc._rows_dirty
    rc.check_capacity()
    for later in steps[1:]:
        _assert_same(later, steps[0], kind)
    per_step = ["fused_project_bwd"] if kind == "sort in forward" else ["fused_bin", "fused_project_bwd"]
    assert calls == per_step * 3, calls
