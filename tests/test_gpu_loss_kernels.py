"""GPU: the kernels that hand the pose step its gradient -- loss_block / k_loss_fused (gsl_tracking_loss), the four
k_normal_* kernels (gsl_normal_loss) and k_pack_pose_reduce -- through the C ABI against the float64 reference of
tests/loss_ref.py, at image borders, tile seams, strips of any rows and loop lengths past one trip.

Every case first shows on the CPU that its input sits on no sign tie (float32 torch against float64 torch,
loss_ref.assert_no_sign_tie); the comparison then counts every pixel, with the bounds of
test_fused_loss_kernel_matches_autograd_loss and test_fused_normal_loss_kernel_matches_autograd_loss.  The NaN that some
cases put outside a strip's rows is data a strip rank never renders and the kernels must not use: no index depends on it."""
import ctypes
import functools

import pytest
import torch

from tests import loss_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -123.25  # prefill of everything a kernel writes: what it leaves alone comes back bit-unchanged


def _lib():
    from gsplatloc_amd._lib import load_library
    return load_library()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _case(W, H, r0, r1, normal, seed=5):
    """(depth, target, reference) of one launch, computed once and shared (never modified); the tie guard runs here."""
    depth, target = R.loss_inputs(W, H, seed=seed, near_target=normal)
    lam_d, lam_n = (R.NORMAL_LAMBDA_DEPTH, R.NORMAL_LAMBDA) if normal else (R.LAMBDA_DEPTH, 0.0)
    ref = R.evaluate(depth, target, r0, r1, lam_d, 1 - lam_d - lam_n, lam_n)
    R.assert_no_sign_tie(depth, target, r0, r1, lam_d, 1 - lam_d - lam_n, lam_n, ref=ref, label=f"{W}x{H} rows {r0}:{r1}")
    return depth, target, ref


def _render(depth, D, seed=9):
    """[H,W,D] with the depth image in the last channel and U(0,1) colours in the others"""
    H, W = depth.shape
    r = torch.rand(H, W, D, generator=torch.Generator().manual_seed(seed))
    r[..., D - 1] = depth
    return r.to(DEV)


def _nan_outside(t, r0, r1):
    """a copy with NaN in every row outside [r0 - 1, r1 + 1)"""
    out = t.clone()
    out[:max(r0 - 1, 0)] = float("nan")
    out[r1 + 1:] = float("nan")
    return out


def _launch(render, gt, r0, r1, normal=False, ws_fill=0.0):
    """gsl_tracking_loss (+ gsl_normal_loss, as the tracker calls them) on sentinel-filled outputs -> raw outputs."""
    from gsplatloc_amd._lib import check, ptr
    lib = _lib()
    H, W, D = render.shape
    lam_d, lam_n = (R.NORMAL_LAMBDA_DEPTH, R.NORMAL_LAMBDA) if normal else (R.LAMBDA_DEPTH, 0.0)
    v = torch.full((H, W, D), SENT, device=DEV)
    nb = lib.gsl_loss_n_partials(W, H, r0, r1)
    partials = torch.full((nb + 1, 2), SENT, device=DEV)  # one row more than the kernel may write
    n_host = ctypes.c_int(-1)
    ws_bytes = lib.gsl_loss_ws_bytes(W, H)
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=DEV)
    check(lib.gsl_tracking_loss(ptr(render), D, ptr(gt), W, H, r0, r1, lam_d, 1 - lam_d - lam_n, ptr(v), ptr(partials),
                                ctypes.addressof(n_host), ptr(ws), ws_bytes, None), "gsl_tracking_loss")
    nsum = None
    if normal:
        fx, fy, cx, cy = R.intrinsics(W, H)
        nws_bytes = lib.gsl_normal_ws_bytes(W, H)
        assert nws_bytes % 4 == 0
        nws = torch.full((nws_bytes // 4,), ws_fill, device=DEV)
        nsum = torch.full((1,), SENT, device=DEV)
        check(lib.gsl_normal_loss(ptr(render), D, ptr(gt), W, H, r0, r1, fx, fy, cx, cy, lam_n, ptr(v), ptr(nsum),
                                  ptr(nws), nws_bytes, None), "gsl_normal_loss")
    torch.cuda.synchronize()
    assert n_host.value == nb, (n_host.value, nb)
    assert float(partials[nb].max()) == SENT and float(partials[nb].min()) == SENT
    return dict(v=v, partials=partials[:nb], nsum=nsum, rows=(r0, r1))


def _result(out, normal=False):
    """The launch as a LossResult (rows it does not write count as zero), after the checks on what it must leave alone:
    every channel but the last, and the depth channel outside [r0 - 1, r1 + 1), bit-unchanged."""
    v, (r0, r1) = out["v"], out["rows"]
    H, W, D = v.shape
    sent = torch.full_like(v, SENT)
    assert _same_bits(v[..., :D - 1], sent[..., :D - 1]), "a channel other than the depth channel was written"
    h0, h1 = (max(r0 - 1, 0), min(r1 + 1, H)) if r1 > r0 else (0, 0)
    assert _same_bits(v[:h0], sent[:h0]) and _same_bits(v[h1:], sent[h1:]), "rows outside the halo were written"
    grad = torch.zeros(H, W, dtype=torch.float64)
    grad[h0:h1] = v[h0:h1, :, D - 1].double().cpu()
    sums = out["partials"].double().sum(0).cpu()  # the partials count as their sum
    ds, es = float(sums[0]), float(sums[1])
    lam_d, lam_n = (R.NORMAL_LAMBDA_DEPTH, R.NORMAL_LAMBDA) if normal else (R.LAMBDA_DEPTH, 0.0)
    total = (lam_d * ds + (1 - lam_d - lam_n) * es) / (W * H)
    cs = None
    if normal:
        cs = float(out["nsum"])
        total += lam_n * ((r1 - r0) / H - cs / (3.0 * H))
    return R.LossResult(total, ds, es, grad, cs)


def _report(tag, errs):
    print(f"[loss-kernels] {tag}: " + ", ".join(f"{k} {e:.2e} (<= {b:.0e})" for k, (e, b) in errs.items()))


def _check_partition(whole, parts, normal, tag):
    """The strips' sums, totals and gradients add up to the whole-image launch's (same bounds)."""
    acc = R.LossResult(sum(p.total for p in parts), sum(p.depth_sum for p in parts), sum(p.edge_sum for p in parts),
                       sum(p.grad for p in parts))
    _report(tag, R.assert_loss_close(acc, whole, normal, tag))


@pytest.mark.parametrize("D", [1, 2, 4])
@pytest.mark.parametrize("W,H", R.WHOLE_SHAPES)
def test_tracking_loss_whole_image(W, H, D):
    """Images of one pixel, below the 3x3 stencil, below a block, one pixel wide or high, exact multiples of 16 and odd
    sizes; one channel (the tracker's own "ED" mode), two and four."""
    depth, target, ref = _case(W, H, 0, H, False)
    got = _result(_launch(_render(depth, D), target.to(DEV), 0, H))
    _report(f"whole {W}x{H} D={D}", R.assert_loss_close(got, ref, False, f"{W}x{H} D={D}"))


@pytest.mark.parametrize("D", [1, 4])
@pytest.mark.parametrize("W,H", R.STRIP_SHAPES)
def test_tracking_loss_strips(W, H, D):
    """Every single tile row, every pair of tile rows, {first, rest} and rows that start or end inside a tile: value and
    gradient on the rows [r0 - 1, r1 + 1), nothing written outside them, nothing read outside them (NaN there), and
    the strips of a partition add up to the whole-image launch."""
    depth, target, _ = _case(W, H, 0, H, False)
    render, gt = _render(depth, D), target.to(DEV)
    whole = _result(_launch(render, gt, 0, H))
    done = {}
    for r0, r1 in R.strips_of(W, H):
        ref = _case(W, H, r0, r1, False)[2]
        out = _launch(render, gt, r0, r1)
        got = done[(r0, r1)] = _result(out)
        _report(f"strip {W}x{H} D={D} rows {r0}:{r1}", R.assert_loss_close(got, ref, False, f"{W}x{H} rows {r0}:{r1}"))
        blind = _launch(_nan_outside(render, r0, r1), _nan_outside(gt, r0, r1), r0, r1)
        assert _same_bits(blind["v"], out["v"]) and _same_bits(blind["partials"], out["partials"]), (r0, r1)
    for part in R.partitions_of(H):
        _check_partition(whole, [done[s] for s in part], False, f"partition {W}x{H} D={D} {part}")
    for r in (0, 16, H):  # an empty strip writes nothing (the sentinel checks of _result) and is no error
        empty = _result(_launch(render, gt, r, r))
        assert empty.depth_sum == 0.0 and empty.edge_sum == 0.0 and float(empty.grad.abs().max()) == 0.0


def test_tracking_loss_exact_ties():
    """render == target on a 20x20 patch that lies across tile seams of a 48x48 image: sign(0) = 0 for the depth term
    and for the edge term of every pixel whose stencil stays on the patch: two pixels in from the patch's rim the
    gradient is exactly zero, while the two outer rings still receive their neighbours' edge terms.  And an all-zero
    depth image: everything masked, sums and gradient exactly zero."""
    W = H = 48
    depth, target = R.loss_inputs(W, H)
    py, px = slice(14, 34), slice(20, 40)  # clear of the hole of zeros
    assert bool((depth[py, px] != 0).all())
    depth = depth.clone()
    depth[py, px] = target[py, px]
    ref = R.evaluate(depth, target, 0, H, R.LAMBDA_DEPTH, R.LAMBDA_EDGE)
    R.assert_no_sign_tie(depth, target, 0, H, R.LAMBDA_DEPTH, R.LAMBDA_EDGE, ref=ref, label="ties")
    assert float(ref.grad[16:32, 22:38].abs().max()) == 0.0 and float(ref.grad[14, 20:40].abs().max()) > 0.0
    for D in (1, 4):
        got = _result(_launch(_render(depth, D), target.to(DEV), 0, H))
        _report(f"ties D={D}", R.assert_loss_close(got, ref, False, "ties"))
        on_patch = float((got.grad[py, px] - ref.grad[py, px]).abs().max())
        assert on_patch <= R.TOL_GRAD * float(ref.grad.abs().max()), on_patch
        assert float(got.grad[16:32, 22:38].abs().max()) == 0.0
        zero = _result(_launch(_render(torch.zeros(H, W), D), target.to(DEV), 0, H))
        assert zero.depth_sum == 0.0 and zero.edge_sum == 0.0 and float(zero.grad.abs().max()) == 0.0


@pytest.mark.parametrize("D", [1, 4])
@pytest.mark.parametrize("W,H", R.NORMAL_SHAPES)
def test_normal_loss(W, H, D):
    """gsl_tracking_loss then gsl_normal_loss: rows wider than one trip of the 256-thread row loop (257, 300), more owned
    rows than one trip of the row-sum loop (270), images below the stencil; a workspace full of NaN changes no bit;
    {first, rest} strips add up and do not see what lies outside their halo."""
    depth, target, ref = _case(W, H, 0, H, True)
    render, gt = _render(depth, D), target.to(DEV)
    out = _launch(render, gt, 0, H, normal=True)
    whole = _result(out, normal=True)
    _report(f"normal whole {W}x{H} D={D}", R.assert_loss_close(whole, ref, True, f"normal {W}x{H}"))
    stale = _launch(render, gt, 0, H, normal=True, ws_fill=float("nan"))
    assert _same_bits(stale["v"], out["v"]) and _same_bits(stale["nsum"], out["nsum"])
    if (W, H) not in R.NORMAL_STRIP_SHAPES:
        return
    parts = []
    for r0, r1 in R.first_rest(H):
        sref = _case(W, H, r0, r1, True)[2]
        sout = _launch(render, gt, r0, r1, normal=True)
        parts.append(_result(sout, normal=True))
        _report(f"normal strip {W}x{H} D={D} rows {r0}:{r1}",
                R.assert_loss_close(parts[-1], sref, True, f"normal {W}x{H} rows {r0}:{r1}"))
        blind = _launch(_nan_outside(render, r0, r1), _nan_outside(gt, r0, r1), r0, r1, normal=True, ws_fill=float("nan"))
        for k in ("v", "partials", "nsum"):
            assert _same_bits(blind[k], sout[k]), (k, r0, r1)
    _check_partition(whole, parts, True, f"normal partition {W}x{H} D={D}")


@pytest.mark.parametrize("with_normal_sum", [True, False])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1200])
def test_pack_pose_reduce(n, with_normal_sum):
    """The v_viewmat path of gsl_pack_pose_reduce with fewer, exactly and more partials than its 256 threads (a 640x480
    frame has 1200 blocks).  A float32 sum of n positive terms in any order is within n 2^-24 relative of the exact one."""
    from gsplatloc_amd._lib import check, ptr
    g = torch.Generator().manual_seed(21 + n)
    vv = (torch.rand(16, generator=g) - 0.5).to(DEV)
    partials = torch.rand(max(n, 1), 2, generator=g)
    nsum = torch.tensor([1.75 + n], device=DEV) if with_normal_sum else None
    out = torch.full((16,), float("nan"), device=DEV)
    p_dev = partials.to(DEV)
    check(_lib().gsl_pack_pose_reduce(ptr(vv), None, 0, None, None, ptr(p_dev), n, ptr(nsum), ptr(out), None), "pack")
    torch.cuda.synchronize()
    assert _same_bits(out[:12], vv[:12])
    want = partials[:n].double().sum(0)
    for c in range(2):
        err = abs(float(out[12 + c]) - float(want[c]))
        assert err <= n * 2.0 ** -24 * float(want[c]), (c, err, float(want[c]))
    assert float(out[14]) == (1.75 + n if with_normal_sum else 0.0)
    assert _same_bits(out[15:], torch.zeros(1, device=DEV))
