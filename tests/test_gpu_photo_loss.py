"""GPU: gsl_photo_loss (csrc/photo.hip: k_photo_stats, k_photo_grad) through the C ABI against the float64 reference of
tests/photo_ref.py, at the smallest shapes where the apron, the block seams and the ragged edges can go wrong:

    11x11  one window, one partial block
    16x16  one full block; every pixel with a window lies on the edge of the valid region
    27x21  partial blocks on both axes, windows that straddle the seam
    48x33  3x3 blocks: an interior block with all eight neighbours, a last block row of a single pixel row

Outputs and workspace are prefilled with a sentinel (NaN in the workspace), then one synchronise.  tests/
test_photo_loss_cpu.py shows that these inputs sit on no tie and that the reference's own float32 evaluation is within
3.3e-6 of the float64 gradient: the bound of 1e-5 leaves that three-fold room."""
import functools

import pytest
import torch

from tests import photo_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -123.25


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _case(W, H, kind):
    """(colours, depth, pixels, reference) of one launch, computed once and shared (never modified)"""
    colors, depth, pixels = R.photo_inputs(W, H, kind)
    ref = R.evaluate(colors, depth, pixels)
    R.assert_no_tie(ref, f"{W}x{H} {kind}")
    return colors, depth, pixels, ref


def _launch(colors, depth, pixels, rgb_lambda=R.RGB_LAMBDA, ssim_lambda=R.SSIM_LAMBDA, poison=False):
    """One gsl_photo_loss on sentinel-filled outputs -> (v_render [H,W,4], photo_sums [3]) on the device."""
    from gsplatloc_amd._lib import check, load_library, ptr
    lib = load_library()
    H, W = depth.shape
    render = torch.cat([colors, depth[..., None]], -1).contiguous().to(DEV)
    px = pixels.contiguous().to(DEV)
    v = torch.full((H, W, 4), SENT, device=DEV)
    sums = torch.full((4,), SENT, device=DEV)  # one more than the kernel may write
    ws_bytes = lib.gsl_photo_ws_bytes(W, H)
    assert ws_bytes % 4 == 0 and ws_bytes > 0
    ws = torch.full((ws_bytes // 4 + 4,), float("nan"), device=DEV)
    if poison:
        check(lib.gsl_dev_poison_lds(0xFFFFFFFF, None), "gsl_dev_poison_lds")
    check(lib.gsl_photo_loss(ptr(render), 4, ptr(px), W, H, rgb_lambda, ssim_lambda, ptr(v), ptr(sums), ptr(ws),
                             ws_bytes, None), "gsl_photo_loss")
    torch.cuda.synchronize()
    assert float(sums[3]) == SENT
    assert bool(torch.isnan(ws[ws_bytes // 4:]).all()), "written past the workspace"
    assert _same_bits(v[..., 3], torch.full((H, W), SENT, device=DEV)), "the depth channel of v_render was written"
    return v, sums[:3]


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("W,H", R.SHAPES)
def test_photo_loss_matches_the_reference(W, H, kind):
    colors, depth, pixels, ref = _case(W, H, kind)
    v, sums = _launch(colors, depth, pixels)
    count, l1_sum, s_sum = (float(x) for x in sums.double().cpu())
    got = v[..., :3].double().cpu()
    e_l1, e_s, e_g = R.rel(l1_sum, ref.l1_sum), R.rel(s_sum, ref.s_sum), R.grad_error(got, ref.grad)
    print(f"[photo-kernels] {W}x{H} {kind}: sum|c-p| {e_l1:.2e}, sum S {e_s:.2e} (<= {R.TOL_SUM:.0e}), "
          f"gradient {e_g:.2e} (<= {R.TOL_GRAD:.0e})")
    assert count == float((depth != 0).sum()) == ref.count
    assert e_l1 <= R.TOL_SUM and e_s <= R.TOL_SUM
    assert e_g <= R.TOL_GRAD
    masked = (depth == 0).to(DEV)
    assert _same_bits(v[..., :3][masked], torch.zeros_like(v[..., :3][masked])), "a masked pixel has a gradient"


def test_photo_loss_is_deterministic_and_reads_no_stale_lds():
    colors, depth, pixels, _ = _case(27, 21, "noise")
    v0, s0 = _launch(colors, depth, pixels)
    v1, s1 = _launch(colors, depth, pixels)
    assert _same_bits(v0, v1) and _same_bits(s0, s1), "two launches differ"
    v2, s2 = _launch(colors, depth, pixels, poison=True)
    assert _same_bits(v0, v2) and _same_bits(s0, s2), "LDS left by another kernel changed the result"


def test_photo_loss_of_a_fully_masked_frame():
    colors, depth, pixels, _ = _case(27, 21, "noise")
    W, H = 27, 21
    v, sums = _launch(colors, torch.zeros_like(depth), pixels)
    assert sums.tolist() == [0.0, 0.0, float(3 * (H - 10) * (W - 10))]
    assert _same_bits(v[..., :3], torch.zeros(H, W, 3, device=DEV))


def test_photo_loss_of_constant_images():
    """sigma^2 = 0 in every window: the clamp's edge.  The sums are compared; the gradient only has to be finite --
    which side of the clamp a rounding lands on legitimately switches the d / d sigma^2 term on or off."""
    W, H = 27, 21
    colors = torch.tensor([0.3, 0.55, 0.8]).expand(H, W, 3).contiguous()
    pixels = torch.tensor([0.35, 0.5, 0.1]).expand(H, W, 3).contiguous()
    depth = torch.full((H, W), 1.5)
    ref = R.evaluate(colors, depth, pixels)
    v, sums = _launch(colors, depth, pixels)
    count, l1_sum, s_sum = (float(x) for x in sums.double().cpu())
    print(f"[photo-kernels] constant images: sum|c-p| {R.rel(l1_sum, ref.l1_sum):.2e}, sum S {R.rel(s_sum, ref.s_sum):.2e}")
    assert bool(torch.isfinite(sums).all()) and bool(torch.isfinite(v[..., :3]).all())
    assert count == W * H
    assert R.rel(l1_sum, ref.l1_sum) <= R.TOL_SUM and R.rel(s_sum, ref.s_sum) <= R.TOL_SUM
