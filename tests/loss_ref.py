"""Plain torch reference (autograd, float64 by default) of the tracker's loss for ARBITRARY owned pixel rows [r0, r1), the
inputs, shapes and strips the loss-kernel tests use, and the comparator those tests judge a result with.

    tracking(d, g, r0, r1, depth_w, edge_w) = (depth_w * sum_own |d*m - g*m| + edge_w * sum_own |S(d*m) - S(g*m)|) / (W*H)

m = (d != 0) carries no gradient, S is my_gsplat.loss.sobel of the WHOLE image (masked to the owned rows afterwards) and
both sums are returned as well.  The normal-consistency share is the one parallel.strip_tracking_loss defines: the row
cosines of the owned rows, with everything outside [r0 - 1, r1 + 1) zeroed first.  tests/test_loss_ref_cpu.py ties all
of this to the project's own definitions and shows that the comparator rejects three seeded defects
(``defect=...``); tests/test_gpu_loss_kernels.py compares the HIP kernels with it."""
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor

from gsplatloc_amd.my_gsplat.geometry import depth_to_normal
from gsplatloc_amd.my_gsplat.loss import sobel
from gsplatloc_amd.synthetic import replica_intrinsics

# the project's own bounds (test_fused_loss_kernel_matches_autograd_loss, test_fused_normal_loss_kernel_matches_...)
TOL_DEPTH_SUM = 1e-5     # relative
TOL_EDGE_SUM = 1e-4      # relative
TOL_GRAD = 1e-5          # max |v - ref| <= this * max |ref|, tracking term alone
TOL_GRAD_NORMAL = 2e-4   # the same with the normal term
TOL_TOTAL_NORMAL = 2e-5  # relative, total value with the normal term
# float32 torch against float64 torch on the same input (no sign tie in it): a tenth of the gradient bound of the
# tracking term, a twentieth of the bound with the normal term
GUARD_GRAD = 1e-6
GUARD_GRAD_NORMAL = 1e-5

DEFECTS = ("zero_pad", "no_halo_grad", "own_pixels")

WHOLE_SHAPES = [(1, 1), (2, 2), (3, 3), (15, 1), (1, 40), (16, 16), (32, 48), (17, 33), (33, 18), (75, 52)]  # (W, H)
STRIP_SHAPES = [(75, 52), (33, 18), (32, 48)]
UNALIGNED_ROWS = {(75, 52): [(5, 23), (23, 24), (51, 52)]}
NORMAL_SHAPES = [(75, 52), (300, 20), (257, 17), (20, 270), (2, 5), (5, 2), (3, 3), (1, 4)]
NORMAL_STRIP_SHAPES = NORMAL_SHAPES[:4]
LAMBDA_DEPTH, LAMBDA_EDGE = 0.8, 0.2                 # the tracker's weights
NORMAL_LAMBDA_DEPTH, NORMAL_LAMBDA = 0.7, 0.1       # with the normal term: edge weight 1 - 0.7 - 0.1


def tile_rows(H: int) -> int:
    return (H + 15) // 16


def rows_of(t0: int, t1: int, H: int) -> Tuple[int, int]:
    """pixel rows of the tile rows [t0, t1)"""
    return t0 * 16, min(t1 * 16, H)


def first_rest(H: int) -> List[Tuple[int, int]]:
    """the partition {first tile row, all the others} in pixel rows"""
    return [rows_of(0, 1, H), rows_of(1, tile_rows(H), H)]


def strips_of(W: int, H: int) -> List[Tuple[int, int]]:
    """Every single tile row, every contiguous pair of tile rows, {first, rest}, and the shape's unaligned rows."""
    th = tile_rows(H)
    out = [rows_of(t, t + 1, H) for t in range(th)] + [rows_of(t, t + 2, H) for t in range(th - 1)] + first_rest(H)
    out += UNALIGNED_ROWS.get((W, H), [])
    seen, uniq = set(), []
    for s in out:
        if s not in seen and s[1] > s[0]:
            seen.add(s)
            uniq.append(s)
    return uniq


def partitions_of(H: int) -> List[List[Tuple[int, int]]]:
    """Partitions of the image the additivity checks use: the single tile rows, and {first, rest}."""
    th = tile_rows(H)
    parts = [[rows_of(t, t + 1, H) for t in range(th)]]
    if th > 2:
        parts.append(first_rest(H))
    return parts


def loss_inputs(W: int, H: int, seed: int = 5, near_target: bool = False) -> Tuple[Tensor, Tensor]:
    """(depth, target) [H,W] float32, both U(0.5, 3.5) (near_target: depth = target + 0.05 randn, the input of the
    normal-term tests).  Images larger than 8x8 get a rectangle of zeros that crosses the first tile seam where the
    image has one, and a zero first column: mask = (depth != 0)."""
    g = torch.Generator().manual_seed(seed)
    target = torch.rand(H, W, generator=g, dtype=torch.float64) * 3 + 0.5
    if near_target:
        depth = target + 0.05 * torch.randn(H, W, generator=g, dtype=torch.float64)
    else:
        depth = torch.rand(H, W, generator=g, dtype=torch.float64) * 3 + 0.5
    if W > 8 and H > 8:
        y0, x0 = H // 10, W // 8 + 1
        depth[y0:y0 + max(4, H // 4), x0:x0 + max(2, W // 4)] = 0.0
        depth[:, 0] = 0.0
    return depth.float(), target.float()


def intrinsics(W: int, H: int) -> Tuple[float, float, float, float]:
    K = replica_intrinsics(W, H, dtype=torch.float64)
    return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])


def _sobel_zero_pad(x: Tensor, eps: float = 1e-6) -> Tensor:
    """defect (a): my_gsplat.loss.sobel with zero padding in place of replicate padding"""
    b, c, h, w = x.shape
    col = torch.tensor([1.0, 2.0, 1.0], dtype=x.dtype)
    dif = torch.tensor([-1.0, 0.0, 1.0], dtype=x.dtype)
    pair = torch.stack([torch.outer(col, dif), torch.outer(dif, col)]) / 8.0
    planes = F.pad(x.reshape(b * c, 1, h, w), (1, 1, 1, 1), mode="constant", value=0.0)
    gx, gy = F.conv2d(planes, pair[:, None]).unbind(dim=1)
    return torch.sqrt(gx * gx + gy * gy + eps).reshape(b, c, h, w)


def tracking(d: Tensor, g: Tensor, r0: int, r1: int, depth_w: float, edge_w: float, defect: Optional[str] = None):
    """(total, sum_own |d m - g m|, sum_own |S(d m) - S(g m)|) of the depth images d, g [H,W], differentiable in d."""
    H, W = d.shape
    assert 0 <= r0 <= r1 <= H
    m = (d != 0).to(d.dtype).detach()
    dm, gm = d * m, g * m
    S = _sobel_zero_pad if defect == "zero_pad" else sobel
    depth_sum = (dm[r0:r1] - gm[r0:r1]).abs().sum()
    edge_sum = (S(dm[None, None])[0, 0, r0:r1] - S(gm[None, None])[0, 0, r0:r1]).abs().sum()
    pixels = float((r1 - r0) * W) if defect == "own_pixels" and r1 > r0 else float(W * H)  # defect (c)
    return (depth_w * depth_sum + edge_w * edge_sum) / pixels, depth_sum, edge_sum


def normal_share(d: Tensor, g: Tensor, r0: int, r1: int, normal_w: float, K: Tensor):
    """(share of the loss, sum of the owned rows' cosines): normal_w * ((r1 - r0) / H - cos_sum / (3 H))."""
    H, W = d.shape
    keep = torch.zeros_like(d)
    keep[max(r0 - 1, 0):min(r1 + 1, H)] = 1.0
    m = (d != 0).to(d.dtype).detach() * keep
    na, nb = depth_to_normal(d * m, K), depth_to_normal(g * m, K)
    cos_sum = F.cosine_similarity(na[r0:r1], nb[r0:r1], dim=1).sum()
    return normal_w * ((r1 - r0) / float(H) - cos_sum / (3.0 * H)), cos_sum


@dataclass
class LossResult:
    total: float
    depth_sum: float
    edge_sum: float
    grad: Tensor                     # [H,W] float64: d total / d depth
    cos_sum: Optional[float] = None  # sum of the owned rows' cosines (normal term only)


def evaluate(depth: Tensor, target: Tensor, r0: int, r1: int, depth_w: float, edge_w: float, normal_w: float = 0.0,
             dtype=torch.float64, defect: Optional[str] = None) -> LossResult:
    """Value and gradient of this strip's share, computed in ``dtype`` from the float32 images the kernels see
    (normal_w != 0: with the normal term, intrinsics replica_intrinsics(W, H))."""
    assert defect is None or defect in DEFECTS
    H, W = depth.shape
    d = depth.to(dtype).clone().requires_grad_()
    g = target.to(dtype)
    total, ds, es = tracking(d, g, r0, r1, depth_w, edge_w, defect)
    cos_sum = None
    if normal_w != 0.0:
        share, cs = normal_share(d, g, r0, r1, normal_w, replica_intrinsics(W, H, dtype=dtype))
        total, cos_sum = total + share, float(cs.detach())
    if total.requires_grad:
        total.backward()
    grad = d.grad.double() if d.grad is not None else torch.zeros(H, W, dtype=torch.float64)
    if defect == "no_halo_grad":  # defect (b)
        grad = grad.clone()
        grad[:r0] = 0.0
        grad[r1:] = 0.0
    return LossResult(float(total.detach()), float(ds.detach()), float(es.detach()), grad, cos_sum)


def _rel(a: float, b: float) -> float:
    return abs(a - b) / abs(b) if b != 0.0 else (0.0 if a == b else float("inf"))


def loss_errors(got: LossResult, ref: LossResult, normal: bool = False) -> Dict[str, Tuple[float, float]]:
    """{quantity: (error, bound)} of a result against the reference, every pixel counted.  Sums and total: relative;
    gradient: max |v - ref| / max |ref|.  A reference of exactly zero admits only zero."""
    gmax = float(ref.grad.abs().max())
    gdiff = float((got.grad.double() - ref.grad).abs().max())
    gerr = gdiff / gmax if gmax != 0.0 else (0.0 if gdiff == 0.0 else float("inf"))
    out = {"depth_sum": (_rel(got.depth_sum, ref.depth_sum), TOL_DEPTH_SUM),
           "edge_sum": (_rel(got.edge_sum, ref.edge_sum), TOL_EDGE_SUM),
           "grad": (gerr, TOL_GRAD_NORMAL if normal else TOL_GRAD)}
    if normal:
        out["total"] = (_rel(got.total, ref.total), TOL_TOTAL_NORMAL)
    return out


def assert_loss_close(got: LossResult, ref: LossResult, normal: bool = False, label: str = ""):
    """THE comparator of the loss-kernel tests; returns the errors it measured."""
    errs = loss_errors(got, ref, normal)
    bad = {k: v for k, v in errs.items() if not v[0] <= v[1]}
    assert not bad, f"{label}: " + ", ".join(f"{k} {e:.3e} > {b:.0e}" for k, (e, b) in bad.items())
    return errs


def assert_no_sign_tie(depth: Tensor, target: Tensor, r0: int, r1: int, depth_w: float, edge_w: float,
                       normal_w: float = 0.0, ref: Optional[LossResult] = None, label: str = "") -> float:
    """The float32 torch evaluation of the reference agrees with the float64 one: the input sits on no sign tie (a
    sign(S_d - S_g) or sign(d - g) that float32 rounding flips moves the gradient by ~1/(W H), far above the bound)."""
    ref = ref if ref is not None else evaluate(depth, target, r0, r1, depth_w, edge_w, normal_w)
    lo = evaluate(depth, target, r0, r1, depth_w, edge_w, normal_w, dtype=torch.float32)
    err = loss_errors(lo, ref, normal_w != 0.0)["grad"][0]
    bound = GUARD_GRAD_NORMAL if normal_w != 0.0 else GUARD_GRAD
    assert err <= bound, f"{label}: float32 against float64 reference gradient {err:.2e} > {bound:.0e}: change the seed"
    return err
