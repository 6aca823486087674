"""Plain torch reference (autograd, float64 by default) of the tracker's photometric term, the inputs and shapes the
photometric tests use, and the guard that an input sits on no tie.

    m     = (depth != 0)  (no gradient),   c = colours * m,   p = pixels * m
    l1    = sum |c - p| / (sum m + 1e-8)                        sum m counts pixels, the numerator all three channels
    ssim  = mean over channels and the (H-10)(W-10) windows inside the image of
            S = (2 mx my + C1)(2 sxy + C2) / ((mx^2 + my^2 + C1)(sx + sy + C2)),  C1 = 1e-4, C2 = 9e-4,
            mx = w*c, my = w*p, sx = max(w*c^2 - mx^2, 0), sy likewise, sxy = w*(c p) - mx my
    photo = (1 - ssim_lambda) l1 + ssim_lambda (1 - ssim);      evaluate() differentiates rgb_lambda * photo

The window w = g (x) g (11 taps of a sigma = 1.5 Gaussian, normalised) is applied here as ONE unfolded 121-tap sum per
window position -- no conv2d, no separable passes -- so that it shares no code path with my_gsplat.loss or the kernels."""
from dataclasses import dataclass
from typing import Tuple

import torch
from torch import Tensor

WIN, SIGMA, C1, C2 = 11, 1.5, 1e-4, 9e-4
SHAPES = [(11, 11), (16, 16), (27, 21), (48, 33)]  # (W, H)
KINDS = ("noise", "near")
RGB_LAMBDA, SSIM_LAMBDA = 0.2, 0.5
TOL_SUM = 1e-5    # relative, sum |c - p| and sum S
TOL_GRAD = 1e-5   # max |v - ref| <= this * max |ref|  (TOL_GRAD of tests/loss_ref.py)
# what an input has to keep clear of (assert_no_tie), and what the float32 evaluation of this very reference may differ
# from the float64 one by on the inputs of the tests (tests/test_photo_loss_cpu.py)
TIE_DIFF, TIE_CLAMP = 1e-6, 1e-6
MIN_DIFF = 1.1e-5
GUARD_GRAD, GUARD_SSIM = 3.3e-6, 4e-7


def window(dtype=torch.float64) -> Tensor:
    k = torch.arange(WIN, dtype=torch.float64) - (WIN - 1) / 2
    g = torch.exp(-(k / SIGMA) ** 2 / 2)
    g = g / g.sum()
    return torch.outer(g, g).to(dtype)


def _windows(x: Tensor) -> Tensor:
    """[3,H,W] -> [3,H-10,W-10,11,11]: every 11x11 patch that lies inside the image"""
    return x.unfold(1, WIN, 1).unfold(2, WIN, 1)


def _filter(x: Tensor, w: Tensor) -> Tensor:
    return (_windows(x) * w).sum((-1, -2))


def photo_inputs(W: int, H: int, kind: str = "noise", seed: int = 0) -> Tuple[Tensor, Tensor, Tensor]:
    """(colours [H,W,3], depth [H,W], pixels [H,W,3]) float32: pixels ~ U(0,1); colours ~ U(0,1) ("noise") or
    pixels + 0.05 N(0,1) clamped to [0,1] ("near"); depth ~ U(1,2) with a random 15 % of the pixels at 0."""
    assert kind in KINDS
    g = torch.Generator().manual_seed(1000 * W + 10 * H + seed + (0 if kind == "noise" else 5))
    pixels = torch.rand(H, W, 3, generator=g, dtype=torch.float64)
    if kind == "noise":
        colors = torch.rand(H, W, 3, generator=g, dtype=torch.float64)
    else:
        colors = (pixels + 0.05 * torch.randn(H, W, 3, generator=g, dtype=torch.float64)).clamp(0.0, 1.0)
    depth = torch.rand(H, W, generator=g, dtype=torch.float64) + 1.0
    depth[torch.rand(H, W, generator=g) < 0.15] = 0.0
    return colors.float(), depth.float(), pixels.float()


@dataclass
class PhotoResult:
    total: float       # rgb_lambda * photo
    count: float       # sum m
    l1_sum: float      # sum |c - p|
    s_sum: float       # sum S
    l1: float
    ssim: float
    grad: Tensor       # [H,W,3] float64: d total / d colours
    min_diff: float    # smallest |c - p| over the unmasked values
    min_var: float     # smallest w*x^2 - mu^2 over both images (before the clamp)


def photo_terms(colors: Tensor, depth: Tensor, pixels: Tensor):
    """(l1, ssim, count, sum |c - p|, sum S, smallest unclamped variance), differentiable in colours [H,W,3]."""
    H, W, _ = colors.shape
    if H < WIN or W < WIN:
        raise ValueError(f"the {WIN}x{WIN} window needs an image of at least that size")
    m = (depth != 0).to(colors.dtype).detach()
    c = (colors * m[..., None]).permute(2, 0, 1)
    p = (pixels.to(colors.dtype) * m[..., None]).permute(2, 0, 1)
    count, l1_sum = m.sum(), (c - p).abs().sum()
    w = window(colors.dtype)
    mx, my = _filter(c, w), _filter(p, w)
    vx, vy = _filter(c * c, w) - mx * mx, _filter(p * p, w) - my * my
    sxy = _filter(c * p, w) - mx * my
    sx, sy = torch.clamp(vx, min=0.0), torch.clamp(vy, min=0.0)
    S = (2 * mx * my + C1) * (2 * sxy + C2) / ((mx * mx + my * my + C1) * (sx + sy + C2))
    return l1_sum / (count + 1e-8), S.mean(), count, l1_sum, S.sum(), torch.minimum(vx.min(), vy.min())


def evaluate(colors: Tensor, depth: Tensor, pixels: Tensor, rgb_lambda: float = RGB_LAMBDA,
             ssim_lambda: float = SSIM_LAMBDA, dtype=torch.float64) -> PhotoResult:
    """Value and gradient of rgb_lambda * photo, computed in ``dtype`` from the float32 images the kernels see."""
    col = colors.to(dtype).clone().requires_grad_()
    l1, ssim, count, l1_sum, s_sum, min_var = photo_terms(col, depth, pixels.to(dtype))
    total = rgb_lambda * ((1 - ssim_lambda) * l1 + ssim_lambda * (1 - ssim))
    total.backward()
    m = depth != 0
    diff = (colors.double() - pixels.double()).abs()[m]
    return PhotoResult(float(total.detach()), float(count), float(l1_sum.detach()), float(s_sum.detach()),
                       float(l1.detach()), float(ssim.detach()), col.grad.double(),
                       float(diff.min()) if diff.numel() else float("inf"), float(min_var.detach()))


def grad_error(got: Tensor, ref: Tensor) -> float:
    """max |got - ref| / max |ref|, every pixel and channel counted; a reference of exactly zero admits only zero"""
    gmax, gdiff = float(ref.abs().max()), float((got.double() - ref).abs().max())
    return gdiff / gmax if gmax != 0.0 else (0.0 if gdiff == 0.0 else float("inf"))


def rel(a: float, b: float) -> float:
    return abs(a - b) / abs(b) if b != 0.0 else (0.0 if a == b else float("inf"))


def assert_no_tie(ref: PhotoResult, label: str = "") -> None:
    """No sign(c - p) and no clamp that a float32 rounding could flip: either moves the gradient far above the bound."""
    assert ref.min_diff > TIE_DIFF, f"{label}: smallest masked |c - p| {ref.min_diff:.2e}: change the seed"
    assert ref.min_var > TIE_CLAMP, f"{label}: a window variance of {ref.min_var:.2e} sits at the clamp: change the seed"
