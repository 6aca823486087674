"""Tracking losses with the interface of /root/reference/src/my_gsplat/loss.py (compute_depth_loss :10-30,
compute_silhouette_loss :33-59, compute_normal_consistency_loss :62-101), plus the photometric pair the reference
writes out and keeps commented (gs_trainer_total.py:111-123).  kornia.filters.sobel, which the
reference calls at loss.py:51-52, is restated here as one 2-channel convolution.  The tracker's per-iteration
loss does not run through these functions in GraphTracker (csrc/tracker.hip fuses depth L1, Sobel L1 and their
adjoint); they are the autograd form used by PoseTracker and by the tests that check the fused kernel.
"""
from typing import Callable, Dict, Literal

import torch
from torch import Tensor
from torch.nn import functional as F

from .geometry import depth_to_normal

_PIXEL_DISTANCES: Dict[str, Callable[[Tensor, Tensor], Tensor]] = {"l1": F.l1_loss, "mse": F.mse_loss}


def _distance(a: Tensor, b: Tensor, loss_type: str, complaint: str) -> Tensor:
    try:
        return _PIXEL_DISTANCES[loss_type](a, b)
    except KeyError:
        raise ValueError(complaint) from None


def sobel(x: Tensor, normalized: bool = True, eps: float = 1e-6) -> Tensor:
    """Gradient magnitude of every channel of x [B,C,H,W] as kornia.filters.sobel computes it: replicate
    padding by one pixel, the 3x3 Sobel pair (divided by 8 when ``normalized``), sqrt(gx^2 + gy^2 + eps)."""
    b, c, h, w = x.shape
    col = torch.tensor([1.0, 2.0, 1.0], dtype=x.dtype, device=x.device)
    dif = torch.tensor([-1.0, 0.0, 1.0], dtype=x.dtype, device=x.device)
    pair = torch.stack([torch.outer(col, dif), torch.outer(dif, col)])  # d/dx, d/dy
    if normalized:
        pair = pair / 8.0
    planes = F.pad(x.reshape(b * c, 1, h, w), (1, 1, 1, 1), mode="replicate")
    gx, gy = F.conv2d(planes, pair[:, None]).unbind(dim=1)
    return torch.sqrt(gx * gx + gy * gy + eps).reshape(b, c, h, w)


def compute_depth_loss(depth_A: Tensor, depth_B: Tensor, *, loss_type: Literal["l1", "mse"] = "l1") -> Tensor:
    """Mean absolute (or squared) difference of two depth images of any common shape."""
    return _distance(depth_A, depth_B, loss_type, "Invalid loss type. Use 'mse' or 'l1'.")


def compute_silhouette_loss(depth_A: Tensor, depth_B: Tensor, *, loss_type: Literal["l1", "mse"] = "l1") -> Tensor:
    """Distance between the Sobel edge maps of two depth images [B,H,W,1]."""
    assert depth_A.dim() == 4 and depth_B.dim() == 4
    edges = [sobel(d.permute(0, 3, 1, 2)) for d in (depth_A, depth_B)]
    return _distance(edges[0], edges[1], loss_type, "Invalid loss type. Use 'mse', 'l1', or 'huber'.")


def compute_normal_consistency_loss(depth_real: Tensor, depth_rendered: Tensor, *, K: Tensor,
                                    loss_type: Literal["cosine", "l1", "mse"] = "cosine") -> Tensor:
    """Disagreement of the normal maps derived from two depth images [H,W] or [1,H,W] (not used by the
    tracker: its normal_lambda is 0)."""
    normals = [depth_to_normal(d.squeeze(0) if d.dim() == 3 else d, K=K) for d in (depth_real, depth_rendered)]
    if loss_type == "cosine":
        return 1 - F.cosine_similarity(normals[0], normals[1], dim=1).mean()
    return _distance(normals[0], normals[1], loss_type, "Invalid loss type. Use 'cosine', 'l1', or 'mse'.")


SSIM_WINDOW, SSIM_SIGMA, SSIM_C1, SSIM_C2 = 11, 1.5, 0.01 ** 2, 0.03 ** 2  # torchmetrics' defaults, data_range = 1


def _masked_images(colors: Tensor, pixels: Tensor, mask: Tensor):
    """(c, p, m) as [3,H,W] / [3,H,W] / [1,H,W] from [H,W,3] or [1,H,W,3] images and a mask with one channel (or none)."""
    c = colors.reshape(colors.shape[-3:]).permute(2, 0, 1)
    p = pixels.reshape(pixels.shape[-3:]).permute(2, 0, 1).to(c.dtype)
    m = mask.detach().reshape(1, c.shape[1], c.shape[2]).to(c.dtype)
    return c * m, p * m, m


def compute_rgb_l1_loss(colors: Tensor, pixels: Tensor, mask: Tensor) -> Tensor:
    """gs_trainer_total.py:112-116: F.l1_loss(colors * mask, pixels * mask, reduction="sum") / (mask.sum() + 1e-8); the
    mask ([..,H,W,1], no gradient) counts pixels, the numerator sums over the three channels as well."""
    c, p, m = _masked_images(colors, pixels, mask)
    return (c - p).abs().sum() / (m.sum() + 1e-8)


def compute_ssim_loss(colors: Tensor, pixels: Tensor, mask: Tensor) -> Tensor:
    """gs_trainer_total.py:119-123: 1 - StructuralSimilarityIndexMeasure(data_range=1.0) of the masked images, as
    torchmetrics computes it by default: an 11x11 window of a sigma = 1.5 Gaussian per channel, the windows that lie
    inside the image (reflect padding, then the padded rim cropped away), variances clamped at 0, C1 = 0.01^2,
    C2 = 0.03^2, mean over windows and channels."""
    c, p, _ = _masked_images(colors, pixels, mask)
    if c.shape[1] < SSIM_WINDOW or c.shape[2] < SSIM_WINDOW:
        raise ValueError(f"the SSIM window needs an image of at least {SSIM_WINDOW}x{SSIM_WINDOW}, got "
                         f"{c.shape[2]}x{c.shape[1]}")
    # The five window moments are taken in float64 whatever the images' dtype: w*c^2 - mx^2 cancels to 1e-7 of c^2 in
    # float32, which against C2 = 9e-4 is 1e-4 of S on a smooth image (csrc/photo.hip does the same).  The window is
    # applied separably as eleven shifted slices per axis: elementwise kernels only, one fixed order.
    k = torch.arange(SSIM_WINDOW, dtype=torch.float64, device=c.device) - (SSIM_WINDOW - 1) / 2
    g = torch.exp(-0.5 * (k / SSIM_SIGMA) ** 2)
    g = (g / g.sum()).tolist()
    cd, pd = c.double(), p.double()
    planes = torch.stack([cd, pd, cd * cd, pd * pd, cd * pd])           # [5,3,H,W]
    hv, wv = c.shape[1] - SSIM_WINDOW + 1, c.shape[2] - SSIM_WINDOW + 1
    rows = sum(g[i] * planes[..., i:i + wv] for i in range(SSIM_WINDOW))
    mx, my, xx, yy, xy = sum(g[i] * rows[..., i:i + hv, :] for i in range(SSIM_WINDOW))
    sx, sy, sxy = torch.clamp(xx - mx * mx, min=0.0), torch.clamp(yy - my * my, min=0.0), xy - mx * my
    S = (2 * mx * my + SSIM_C1) * (2 * sxy + SSIM_C2) / ((mx * mx + my * my + SSIM_C1) * (sx + sy + SSIM_C2))
    return (1 - S.mean()).to(c.dtype)
