"""Fused single-camera render (host side of csrc/fused_project.hip, fused_project_bwd.hip, raster_px.hip,
raster_g16.hip and raster_det.hip: one file per stage).

``fused_rasterization`` runs ``gsplat.rasterization``'s whole forward in five
launches and its backward in three, for the configuration GsplatLoc uses
(/root/reference/src/my_gsplat/model.py:195-213: one camera, packed=False, 16x16
tiles, no background, SH or RGB colours, any of the five render modes).
``rendering.rasterization`` dispatches here when the call fits and to the stage
operators otherwise.  ``tile_rows=(ty0, ty1)`` restricts binning and compositing to
a strip of tile rows (screen-tile parallelism, ``gsplatloc_amd.parallel``).
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Tuple

import torch
from torch import Tensor

from . import stages
from ._lib import load_library
from .stages import _MODES, MAX_STRIP_TILES, alloc_records, tile_n_bits


class FusedCfg(NamedTuple):
    """What one allocate-per-call render depends on besides its tensors.  Whole frame: (ty0, ty1) = (0, tile rows)."""
    width: int
    height: int
    sh_degree: int  # -1: colours are RGB
    mode: str
    eps2d: float
    near_plane: float
    far_plane: float
    radius_clip: float
    antialiased: bool
    ty0: int
    ty1: int
    want_isect_ids: bool


def _make_cfg(width, height, sh_degree, render_mode, eps2d, near_plane, far_plane, radius_clip, antialiased, tile_rows,
              want_isect_ids) -> FusedCfg:
    ty0, ty1 = tile_rows if tile_rows is not None else (0, (height + 15) // 16)
    assert 0 <= ty0 <= ty1 <= (height + 15) // 16, (ty0, ty1, height)
    return FusedCfg(int(width), int(height), -1 if sh_degree is None else int(sh_degree), render_mode, float(eps2d),
                    float(near_plane), float(far_plane), float(radius_clip), bool(antialiased), int(ty0), int(ty1),
                    bool(want_isect_ids))


def _geometry(cfg: FusedCfg):
    """(channels, ed, colours?, tile columns, tile rows) of a configuration."""
    D, ed = _MODES[cfg.mode]
    return D, ed, D >= 3, (cfg.width + 15) // 16, (cfg.height + 15) // 16


def prep(t, name):
    assert t.is_cuda, f"{name} must live on the GPU (got {t.device}); there is no CPU path"
    assert t.dtype == torch.float32, f"{name} must be float32 (got {t.dtype})"
    return t.contiguous()


def _gsplat_meta(width, height, s, means2d=None) -> Dict:
    """gsplat's meta dict ([1,N,...] views) from the arrays of a render: s maps radii, Q0, Q1, tiles_per_gauss,
    flatten_ids, tile_offsets and, where they are produced, isect_ids."""
    tw, th = (width + 15) // 16, (height + 15) // 16
    Q0, Q1 = s["Q0"], s["Q1"]
    return {
        "camera_ids": None, "gaussian_ids": None,
        "radii": s["radii"][None], "means2d": Q0[None, :, 0:2] if means2d is None else means2d, "depths": Q0[None, :, 2],
        "conics": Q1[None, :, 0:3], "opacities": Q0[None, :, 3],
        "tile_width": tw, "tile_height": th, "tiles_per_gauss": s["tiles_per_gauss"][None],
        "isect_ids": s.get("isect_ids"), "flatten_ids": s["flatten_ids"],
        "isect_offsets": s["tile_offsets"][:-1].reshape(1, th, tw), "width": width, "height": height,
        "tile_size": 16, "n_cameras": 1,
    }


# ---------------------------------------------------------------------------------------------------------------------
# The steps of the allocate-per-call path, once each.  `s` is the state of one render: cfg, N, K_sh, n_isects and the arrays
# projection and binning left.  _FusedRasterization keeps them with save_for_backward; the absgrad nodes share `s` itself.
_SCALARS = ("cfg", "N", "K_sh", "n_isects")
_ARRAYS = ("radii", "Q0", "Q1", "Q2", "comps", "tile_offsets", "flatten_ids", "ws")  # what a backward reads


def _project_and_bin(means, quats, scales, opacities, colors, viewmat, K, cfg: FusedCfg) -> Dict:
    """Records, gsl_fused_project, the intersection count read back, lists, gsl_fused_bin."""
    _, _, rgb, tw, th = _geometry(cfg)
    N, dev, n_tiles = means.shape[0], means.device, tw * th
    f32, i32 = torch.float32, torch.int32
    radii = torch.empty(N, dtype=i32, device=dev)
    Q0, Q1, Q2 = alloc_records(N, rgb, dev)
    comps = torch.empty(N, dtype=f32, device=dev) if cfg.antialiased else None
    tpg = torch.empty(N, dtype=i32, device=dev)
    offs = torch.empty(n_tiles + 1, dtype=i32, device=dev)
    n_is = torch.empty(1, dtype=i32, device=dev)
    ws = torch.empty(load_library().gsl_fused_ws_bytes(N, n_tiles), dtype=torch.uint8, device=dev)
    K_sh = colors.shape[1] if (rgb and cfg.sh_degree >= 0) else 0
    # two-pass binning (no bins): tile sizes are not known in advance
    stages.fused_project(means, quats, scales, opacities, colors if rgb else None, cfg.sh_degree, K_sh, viewmat, K, N,
                         cfg.width, cfg.height, cfg.eps2d, cfg.near_plane, cfg.far_plane, cfg.radius_clip,
                         int(cfg.antialiased), tw, th, cfg.ty0, cfg.ty1, radii, Q0, Q1, Q2, comps, tpg, offs, n_is, ws)
    n_isects = int(n_is.item())  # output sizes depend on it (gsplat syncs at the same point)
    keys = torch.empty(max(n_isects, 1), dtype=torch.int64, device=dev)
    flatten_ids = torch.empty(n_isects, dtype=i32, device=dev)
    isect_ids = torch.empty(n_isects, dtype=torch.int64, device=dev) if cfg.want_isect_ids else None
    stages.fused_bin(Q0, radii, N, tw, th, cfg.ty0, cfg.ty1, tile_n_bits(n_tiles), offs, n_isects, keys,
                     flatten_ids if n_isects else None, ws, isect_ids=isect_ids if n_isects else None)
    return dict(cfg=cfg, N=N, K_sh=K_sh, n_isects=n_isects, radii=radii, Q0=Q0, Q1=Q1, Q2=Q2, comps=comps,
                tiles_per_gauss=tpg, tile_offsets=offs, flatten_ids=flatten_ids, isect_ids=isect_ids, ws=ws)


def _composite_fwd(s):
    """Outputs, hit lists and gsl_fused_raster_fwd: (render, alphas, last_ids, hits, hit_counts)."""
    cfg, n_isects = s["cfg"], s["n_isects"]
    D, ed, _, tw, th = _geometry(cfg)
    W, H, dev, f32, i32 = cfg.width, cfg.height, s["Q0"].device, torch.float32, torch.int32
    make = torch.empty if (cfg.ty0, cfg.ty1) == (0, th) else torch.zeros  # (a strip writes its own tile rows only)
    render = make(H, W, D, dtype=f32, device=dev)
    alphas = make(H, W, 1, dtype=f32, device=dev)
    last_ids = torch.zeros(H, W, dtype=i32, device=dev)
    # per tile and quadrant: the entries it composited (a hit word holds the list index in 28 bits: none beyond that,
    # the backward then tests the blocks geometrically)
    hits = torch.empty(4 * max(n_isects, 1), dtype=i32, device=dev) if max(n_isects, 1) < (1 << 28) else None
    hit_counts = torch.empty(4 * tw * th + 1, dtype=i32, device=dev) if hits is not None else None
    stages.fused_raster_fwd(s["Q0"], s["Q1"], s["Q2"], D, int(ed), W, H, tw, th, cfg.ty0, cfg.ty1, s["tile_offsets"],
                            s["flatten_ids"] if n_isects else None, n_isects, render, alphas, last_ids, 0, H,
                            isect_hits=hits, isect_hit_counts=hit_counts)
    return render, alphas, last_ids, hits, hit_counts


def _composite_bwd(s, outputs, v_render, v_alphas, want_absgrad: bool = False):
    """gsl_fused_raster_bwd into a fresh vacc [N,16] and, asked for, gsl_fused_absgrad into a fresh [N,2]: (vacc,
    absgrad or None).  outputs: what _composite_fwd returned."""
    cfg, n_isects = s["cfg"], s["n_isects"]
    D, ed, _, tw, th = _geometry(cfg)
    render, alphas, last_ids, hits, hit_counts = outputs
    v_render, v_alphas = v_render.contiguous(), v_alphas.contiguous()
    lists = (s["tile_offsets"], s["flatten_ids"] if n_isects else None, n_isects, render, alphas, last_ids, v_render,
             v_alphas)
    vacc = torch.zeros(s["N"], 16, dtype=torch.float32, device=render.device)
    stages.fused_raster_bwd(s["Q0"], s["Q1"], s["Q2"], D, int(ed), cfg.width, cfg.height, tw, th, cfg.ty0, cfg.ty1,
                            *lists, vacc, 0, cfg.height, isect_hits=hits, isect_hit_counts=hit_counts)
    absgrad = None
    if want_absgrad:
        absgrad = torch.zeros(s["N"], 2, dtype=torch.float32, device=render.device)
        stages.fused_absgrad(s["Q0"], s["Q1"], s["Q2"], D, int(ed), cfg.width, cfg.height, tw, th, *lists, absgrad,
                             isect_hits=hits, isect_hit_counts=hit_counts)
    return vacc, absgrad


def _project_bwd(s, inputs, vacc, ni):
    """Gradient tensors, gsl_fused_project_bwd (it consumes vacc), and the needs_input_grad filter: what the backward
    of a node with the inputs (means, quats, scales, opacities, colors, viewmat, K, cfg, state) returns."""
    cfg, N = s["cfg"], s["N"]
    D, _, rgb, tw, th = _geometry(cfg)
    means, quats, scales, opacities, colors, viewmat, K = inputs
    dev, f32 = means.device, torch.float32
    v_means = v_quats = v_scales = v_opac = v_colors = None
    if any(ni[:5]):
        v_means = torch.empty(N, 3, dtype=f32, device=dev)
        v_quats = torch.empty(N, 4, dtype=f32, device=dev)
        v_scales = torch.empty(N, 3, dtype=f32, device=dev)
        v_opac = torch.empty(N, dtype=f32, device=dev)
        if rgb:
            v_colors = torch.empty_like(colors)
    v_viewmat = torch.empty(4, 4, dtype=f32, device=dev) if ni[5] else None
    stages.fused_project_bwd(means, quats, scales, opacities, colors if rgb else None, cfg.sh_degree, s["K_sh"], viewmat,
                             K, N, cfg.width, cfg.height, cfg.eps2d, int(cfg.antialiased), D, s["radii"], s["Q1"],
                             s["comps"], vacc, v_means, v_quats, v_scales, v_opac, v_colors, v_viewmat, s["ws"], tw * th, 1)
    return (v_means if ni[0] else None, v_quats if ni[1] else None, v_scales if ni[2] else None,
            v_opac if ni[3] else None, v_colors if (ni[4] and rgb) else None, v_viewmat, None, None, None)


class _FusedRasterization(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means, quats, scales, opacities, colors, viewmat, K, cfg, meta):
        s = _project_and_bin(means, quats, scales, opacities, colors, viewmat, K, cfg)
        outputs = _composite_fwd(s)
        ctx.save_for_backward(means, quats, scales, opacities, colors if _geometry(cfg)[2] else None, viewmat, K,
                              *(s[k] for k in _ARRAYS), *outputs)
        ctx.scalars = {k: s[k] for k in _SCALARS}
        if meta is not None:
            meta.update(s, last_ids=outputs[2])
        ctx.mark_non_differentiable(outputs[2])
        return outputs[:3]

    @staticmethod
    def backward(ctx, v_render, v_alphas, _v_last):
        saved = ctx.saved_tensors
        s = dict(ctx.scalars, **dict(zip(_ARRAYS, saved[7:-5])))
        vacc, _ = _composite_bwd(s, saved[-5:], v_render, v_alphas)
        return _project_bwd(s, saved[:7], vacc, ctx.needs_input_grad)


# ---------------------------------------------------------------------------------------------------------------------
# absgrad=True on the fused path: the same five launches as _FusedRasterization, split into two autograd nodes so that
# the screen-space means sit in the graph between them (gsplat's means2d: retain_grad() gives .grad, and the compositing
# backward sets .absgrad).  The projection node runs gsl_fused_project + gsl_fused_bin and outputs means2d [1,N,2]; the
# compositing node consumes it, and its backward runs gsl_fused_raster_bwd, then gsl_fused_absgrad, and hands the
# v_xy columns of vacc back as v_means2d.  The rest of vacc travels in the shared `state`; the projection node's
# backward writes the incoming v_means2d (which includes anything else added into means2d) back into those columns
# and runs gsl_fused_project_bwd.
class _FusedProjectNode(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means, quats, scales, opacities, colors, viewmat, K, cfg, state):
        _, _, rgb, _, th = _geometry(cfg)
        assert (cfg.ty0, cfg.ty1) == (0, th), "absgrad renders whole frames only (gsl_fused_absgrad)"
        state.update(_project_and_bin(means, quats, scales, opacities, colors, viewmat, K, cfg), vacc=None)
        ctx.save_for_backward(means, quats, scales, opacities, colors if rgb else None, viewmat, K)
        ctx.state = state
        return state["Q0"][None, :, 0:2].clone()

    @staticmethod
    def backward(ctx, v_means2d):
        s = ctx.state
        vacc, s["vacc"] = s["vacc"], None
        if vacc is None:  # (nothing was composited into the loss: means2d is all the gradient there is)
            vacc = torch.zeros(s["N"], 16, dtype=torch.float32, device=v_means2d.device)
        vacc[:, 0:2].copy_(v_means2d[0])
        return _project_bwd(s, ctx.saved_tensors, vacc, ctx.needs_input_grad)


class _FusedCompositeNode(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means2d, state):
        outputs = _composite_fwd(state)
        state["last_ids"] = outputs[2]
        ctx.save_for_backward(means2d, *outputs)
        ctx.state = state
        ctx.mark_non_differentiable(outputs[2])
        return outputs[:3]

    @staticmethod
    def backward(ctx, v_render, v_alphas, _v_last):
        means2d, *outputs = ctx.saved_tensors
        vacc, absgrad = _composite_bwd(ctx.state, outputs, v_render, v_alphas, want_absgrad=True)
        means2d.absgrad = absgrad[None]  # assigned by every backward, as gsplat does
        ctx.state["vacc"] = vacc  # the projection node's backward consumes it
        return vacc[None, :, 0:2].clone(), None


def fused_absgrad_rasterization(
    means: Tensor, quats: Tensor, scales: Tensor, opacities: Tensor, colors: Tensor, viewmat: Tensor, K: Tensor,
    width: int, height: int, sh_degree: Optional[int] = None, render_mode: str = "RGB", eps2d: float = 0.3,
    near_plane: float = 0.01, far_plane: float = 1e10, radius_clip: float = 0.0, antialiased: bool = False,
    want_isect_ids: bool = True,
) -> Tuple[Tensor, Tensor, Dict]:
    """fused_rasterization (whole frame) with meta["means2d"] [1,N,2] in the autograd graph between projection and
    compositing: after a backward it carries ``.absgrad`` (and ``.grad`` when retained), as gsplat's absgrad=True."""
    cfg = _make_cfg(width, height, sh_degree, render_mode, eps2d, near_plane, far_plane, radius_clip, antialiased, None,
                    want_isect_ids)
    render, alphas, means2d, s = fused_absgrad_apply(
        prep(means, "means"), prep(quats, "quats"), prep(scales, "scales"), prep(opacities, "opacities"),
        prep(colors, "colors"), prep(viewmat, "viewmats"), prep(K, "Ks"), cfg)
    return render, alphas, _gsplat_meta(width, height, s, means2d)


def fused_absgrad_apply(means, quats, scales, opacities, colors, viewmat, K, cfg):
    """The two autograd nodes of the absgrad path on prepared tensors: (render [H,W,X], alphas [H,W,1], means2d [1,N,2],
    the shared state)."""
    state: Dict = {}
    means2d = _FusedProjectNode.apply(means, quats, scales, opacities, colors, viewmat, K, cfg, state)
    render, alphas, _ = _FusedCompositeNode.apply(means2d, state)
    return render, alphas, means2d, state


# ---------------------------------------------------------------------------------------------------------------------
# Drop-in call with a cached RenderContext.  `from gsplat import rasterization` under the reference's loop
# (/root/reference/src/my_gsplat/gs_trainer_total.py:79-267) renders the same N Gaussians at the same size a few hundred
# times per frame: allocating ~15 tensors per call, binning in two passes and reading the intersection count back to
# size them (what gsplat itself does, and what _FusedRasterization above does) made that call allocator- and
# launch-bound (0.43 ms wall for 0.09 ms of kernels at S).  Here the context -- records, bins,
# lists, capacity -- is kept per call signature; a call is 3 launches into freshly allocated OUTPUT tensors (the caller
# owns what it gets; nothing returned aliases the context), one 32-byte status read (overflow flags and count: the
# lists are complete or the call is repeated after growing the buffers), and the backward is 3 launches.
# GSLOC_DROPIN_CACHE=0 selects the allocate-per-call path.
_CTX_CACHE: Dict[tuple, "object"] = {}
_CTX_CACHE_MAX = 4


def _cached_context(key, make):
    rc = _CTX_CACHE.pop(key, None)
    if rc is None:
        rc = make()
        while len(_CTX_CACHE) >= _CTX_CACHE_MAX:
            _CTX_CACHE.pop(next(iter(_CTX_CACHE)))
    _CTX_CACHE[key] = rc  # most recently used last
    return rc


def clear_context_cache() -> None:
    _CTX_CACHE.clear()


class _CachedRasterization(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means, quats, scales, opacities, colors, viewmat, K, rc, meta):
        dev = means.device
        f32, i32 = torch.float32, torch.int32
        inputs = (means, quats, scales, opacities, colors if rc.rgb else None, viewmat, K)
        if rc.keys is None:
            rc.calibrate(*inputs)
        for attempt in range(3):
            # outputs are fresh tensors the caller owns; the kernels write every pixel of the frame
            rc.render = torch.empty(rc.H, rc.W, rc.D, dtype=f32, device=dev)
            rc.alphas = torch.empty(rc.H, rc.W, 1, dtype=f32, device=dev)
            rc.last_ids = torch.empty(rc.H, rc.W, dtype=i32, device=dev)
            why = rc.forward_checked(*inputs)
            if why is None:
                break
            rc.calibrate(*inputs, headroom=1.5 * (attempt + 1))  # the scene moved past the head-room: re-measure, repeat
        else:
            raise RuntimeError(f"rasterization: buffers kept overflowing ({why})")
        ctx.rc, ctx.gen = rc, rc.generation
        ctx.save_for_backward(means, quats, scales, opacities, colors if rc.rgb else torch.empty(0, device=dev), viewmat, K,
                              rc.render, rc.alphas, rc.last_ids)
        if meta is not None:
            meta.update(radii=rc.radii, Q0=rc.Q0, Q1=rc.Q1, tile_offsets=rc.offs, n_isects=rc.last_n_isects,
                        flatten_ids=rc.flatten_ids[:rc.last_n_isects], last_ids=rc.last_ids,
                        tiles_per_gauss=rc.tiles_per_gauss)
        ctx.mark_non_differentiable(rc.last_ids)
        return rc.render, rc.alphas, rc.last_ids

    @staticmethod
    def backward(ctx, v_render, v_alphas, _v_last):
        rc = ctx.rc
        means, quats, scales, opacities, colors, viewmat, K, render, alphas, last_ids = ctx.saved_tensors
        dev = means.device
        f32 = torch.float32
        inputs = (means, quats, scales, opacities, colors if rc.rgb else None, viewmat, K)
        rc.render, rc.alphas, rc.last_ids = render, alphas, last_ids
        if rc.generation != ctx.gen:
            # another forward has used this context since: its records and lists are not this node's any more --
            # run this node's forward again (same inputs: same outputs, rewritten into the saved tensors).  The buffers
            # may have been re-sized for the later call's scene: check, and refuse to build a gradient from truncated lists
            why = rc.forward_checked(*inputs)
            if why is not None:
                raise RuntimeError(f"backward of a stale rasterization node: {why} (a later call with the same signature "
                                   "re-sized the cached context; set GSLOC_DROPIN_CACHE=0 to give every call its own buffers)")
        rc._inputs = inputs
        ni = ctx.needs_input_grad
        full = any(ni[:5])
        N = rc.N
        if full:  # gradient tensors are fresh too
            rc.v_means = torch.empty(N, 3, dtype=f32, device=dev)
            rc.v_quats = torch.empty(N, 4, dtype=f32, device=dev)
            rc.v_scales = torch.empty(N, 3, dtype=f32, device=dev)
            rc.v_opacities = torch.empty(N, dtype=f32, device=dev)
            rc.v_colors = torch.empty_like(colors) if rc.rgb else None
        rc.v_viewmat = torch.empty(4, 4, dtype=f32, device=dev)
        g = rc.backward(v_render.contiguous(), v_alphas.contiguous(), full=full)
        return (g["means"] if ni[0] else None, g["quats"] if ni[1] else None, g["scales"] if ni[2] else None,
                g["opacities"] if ni[3] else None, g["colors"] if (ni[4] and rc.rgb) else None,
                g["viewmat"] if ni[5] else None, None, None, None)


def cached_rasterization(means, quats, scales, opacities, colors, viewmat, K, width, height, sh_degree=None,
                         render_mode="RGB", eps2d=0.3, near_plane=0.01, far_plane=1e10, radius_clip=0.0,
                         antialiased=False) -> Tuple[Tensor, Tensor, Dict]:
    """fused_rasterization through a cached RenderContext (whole frame, one camera).  Same returns; the meta tensors
    (radii, means2d, depths, conics, opacities, tile lists) are VIEWS of the context's buffers: valid until the next
    call with the same signature (GsplatLoc never reads them); isect_ids is not produced."""
    from .context import RenderContext

    N = means.shape[0]
    D, _ = _MODES[render_mode]
    rgb = D >= 3
    deg = -1 if sh_degree is None else int(sh_degree)
    K_sh = colors.shape[1] if (rgb and deg >= 0) else 0
    key = (N, int(width), int(height), render_mode, deg, K_sh, float(eps2d), float(near_plane), float(far_plane),
           float(radius_clip), bool(antialiased), means.device.index)
    rc = _cached_context(key, lambda: RenderContext(
        N, width, height, render_mode, sh_degree=sh_degree, K_sh=K_sh, device=means.device, eps2d=eps2d,
        near_plane=near_plane, far_plane=far_plane, radius_clip=radius_clip, antialiased=antialiased, full_grads=False,
        reorder=False))  # (the drop-in call returns per-Gaussian meta tensors and lists in the caller's order)
    tensors = (means, quats, scales, opacities, colors, viewmat)
    # hit lists only when somebody can back-propagate through this call (geometry.py:117-132 renders under no_grad)
    rc.record_hits = torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in tensors)
    rc.allow_tiny = False  # a splat that outgrew the tiny backward is only known after the backward: not in this API
    rc.full_grads = True  # gradient buffers are allocated per call (owned by the caller), not by the context
    if rc.tiles_per_gauss is None:
        rc.tiles_per_gauss = torch.zeros(N, dtype=torch.int32, device=means.device)
    raw: Dict = {}
    render, alphas, _ = _CachedRasterization.apply(
        prep(means, "means"), prep(quats, "quats"), prep(scales, "scales"), prep(opacities, "opacities"),
        prep(colors, "colors") if rgb else colors, prep(viewmat, "viewmats"), prep(K, "Ks"), rc, raw)
    return render, alphas, _gsplat_meta(width, height, raw)


def fused_supported(N: int, C: int, colors: Tensor, sh_degree: Optional[int], width: int, height: int,
                    tile_size: int, backgrounds, render_mode: str, tile_rows=None) -> bool:
    if C != 1 or tile_size != 16 or backgrounds is not None:
        return False
    tw, th = (width + 15) // 16, (height + 15) // 16
    ty0, ty1 = tile_rows if tile_rows is not None else (0, th)
    if (ty1 - ty0) * tw > MAX_STRIP_TILES:
        return False
    if _MODES[render_mode][0] >= 3:
        if sh_degree is None:
            return colors.dim() == 2 and colors.shape == (N, 3)
        return colors.dim() == 3 and colors.shape[0] == N and colors.shape[2] == 3 and 0 <= sh_degree <= 3
    return True


def fused_rasterization(
    means: Tensor, quats: Tensor, scales: Tensor, opacities: Tensor, colors: Tensor, viewmat: Tensor, K: Tensor,
    width: int, height: int, sh_degree: Optional[int] = None, render_mode: str = "RGB", eps2d: float = 0.3,
    near_plane: float = 0.01, far_plane: float = 1e10, radius_clip: float = 0.0, antialiased: bool = False,
    tile_rows: Optional[Tuple[int, int]] = None, want_isect_ids: bool = True,
) -> Tuple[Tensor, Tensor, Dict]:
    """One camera.  Returns render [H,W,X], alphas [H,W,1], meta (gsplat keys, [1,N,...] views)."""
    cfg = _make_cfg(width, height, sh_degree, render_mode, eps2d, near_plane, far_plane, radius_clip, antialiased,
                    tile_rows, want_isect_ids)
    raw: Dict = {}
    render, alphas, _ = _FusedRasterization.apply(
        prep(means, "means"), prep(quats, "quats"), prep(scales, "scales"), prep(opacities, "opacities"),
        prep(colors, "colors"), prep(viewmat, "viewmats"), prep(K, "Ks"), cfg, raw)
    return render, alphas, _gsplat_meta(width, height, raw)
