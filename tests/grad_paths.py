"""Per-Gaussian gradient checks shared by the GPU gradient tests (test code only: it calls the oracle, adds nothing to it).

oracle_render() runs the oracle's stages (oracle/gsplat_oracle.py: projection, SH, tile intersection, compositing) for
one camera.  With half=True it rounds to float16 exactly what an fp16-staged record holds (RenderContext(staging="fp16"),
gsplatloc_amd/csrc/gsloc_common.h store_half_record): conic a, b, c, the opacity after the anti-aliasing compensation
and the colours after SH and the clamp.  The rounding is straight-through, x + (round(x) - x).detach(): the compositing
kernels differentiate at the rounded values and the projection backward chains that through the float32 projection.
The sort keys and the tile rectangles see the unrounded values, as in the kernels; the centre and the depth feature
stay float32 in the record and are not rounded.

compare_grads() is test_fused_full_gradients' element bound (1e-3 relative plus 1e-4 of the largest entry of that
input's gradient), counted per Gaussian -- a Gaussian is an outlier when any of its elements is outside -- and per
subset of Gaussians, so that a bug confined to a few tiles cannot hide in the whole frame's count.
"""
import torch

from oracle import gsplat_oracle as G

GRAD_RTOL = 1e-3     # element bound: 1e-3 relative ...
GRAD_ATOL = 1e-4     # ... plus 1e-4 of the largest entry of that input's gradient
OUTLIER_FRAC = 1e-2  # outlier Gaussians allowed in a subset of at least MIN_SUBSET Gaussians ...
MIN_SUBSET = 100     # ... and in a smaller one: at most one
MODES = {"RGB": (3, False), "D": (1, False), "ED": (1, True), "RGB+D": (4, False), "RGB+ED": (4, True)}


def half_round(x):
    """x rounded to float16 as the projection kernel rounds it (float32, then to nearest even), gradient of x."""
    return x + (x.float().half().to(x.dtype) - x).detach()


def oracle_render(means, quats, scales, opacities, colors, viewmat, K, W, H, mode, sh_degree=None, antialiased=False,
                  near_plane=0.01, far_plane=1e10, eps2d=0.3, half=False):
    """render [H,W,D] and alphas [H,W,1] of one camera (viewmat [4,4], K [3,3]): the stages of G.rasterization;
    half=True rounds what an fp16-staged record holds."""
    D, ed = MODES[mode]
    Vs, Ks = viewmat[None], K[None]
    radii, means2d, depths, conics, comps = G.fully_fused_projection(
        means, quats, scales, Vs, Ks, W, H, eps2d, near_plane, far_plane, 0.0, calc_compensations=antialiased)
    opac = opacities[None]
    if comps is not None:
        opac = opac * comps
    feats = []
    if D >= 3:
        if sh_degree is None:
            cols = colors[None]
        else:
            dirs = means[None] - torch.linalg.inv(Vs)[:, None, :3, 3]
            cols = torch.clamp_min(G.spherical_harmonics(sh_degree, dirs, colors[None], masks=radii > 0) + 0.5, 0.0)
        feats.append(half_round(cols) if half else cols)
    if D != 3:
        feats.append(depths[..., None])
    if half:
        conics, opac = half_round(conics), half_round(opac)
    tw, th = (W + 15) // 16, (H + 15) // 16
    _, isect_ids, flatten_ids = G.isect_tiles(means2d, radii, depths, 16, tw, th)
    offsets = G.isect_offset_encode(isect_ids, 1, tw, th)
    rc, ra = G.rasterize_to_pixels(means2d, conics, torch.cat(feats, -1), opac, W, H, 16, offsets, flatten_ids)
    if ed:
        rc = torch.cat([rc[..., :-1], rc[..., -1:] / ra.clamp(min=G.ED_ALPHA_CLAMP)], dim=-1)
    return rc[0], ra[0]


def compare_grads(got, want, subsets):
    """got: HIP gradients, want: float64 oracle gradients (name -> [N, ...]; only the names in `want` are compared).
    subsets: name -> index tensor.  Returns (worst, counts, bad): worst[input] = max |g - o| / max |o|,
    counts[subset] = (outlier Gaussians, size, allowed), bad = [N] bool."""
    N = next(iter(want.values())).shape[0]
    bad = torch.zeros(N, dtype=torch.bool)
    worst = {}
    for nm, o in want.items():
        g = got[nm].detach().cpu().double().reshape(N, -1)
        o = o.detach().cpu().double().reshape(N, -1)
        scale = float(o.abs().max())
        err = (g - o).abs()
        bad |= (err > GRAD_RTOL * o.abs() + GRAD_ATOL * scale).any(1)
        worst[nm] = float(err.max()) / max(scale, 1e-300)
    counts = {}
    for name, idx in subsets.items():
        n = int(idx.numel())
        counts[name] = (int(bad[idx].sum()), n, int(OUTLIER_FRAC * n) if n >= MIN_SUBSET else 1)
    return worst, counts, bad


def failing_subsets(counts):
    """The subsets whose outlier count exceeds what they allow."""
    return {k: v for k, v in counts.items() if v[0] > v[2]}


def roll_within(grads, groups):
    """The gradients with the rows of every group rolled by one: each Gaussian gets its neighbour's gradient."""
    out = {}
    for nm, g in grads.items():
        src = g.detach().cpu()
        r = src.clone()
        for idx in groups:
            r[idx] = src[idx].roll(1, 0)
        out[nm] = r
    return out
