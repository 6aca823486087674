"""Scenes and helpers of the staged-route width tests (tests/test_gpu_staged_widths.py, tests/test_staged_widths_cpu.py).
Test code only: inputs, and bookkeeping about the oracle's compositing walk; every reference VALUE comes from
oracle/gsplat_oracle.py.

Two scenes on a 40x24 image (3 x 2 tiles of 16 px; the last tile column and the last tile row are 8 px wide):

  deep    1200 anisotropic splats of sigma ~ 2.5 px and opacity 0.02 .. 0.3.  Every tile list is two to five staging
          batches (256 entries) long, every pixel composites entries beyond the first batch and about four in ten stop on
          the transmittance threshold: the backward's batch trims (t_first, wave_final, block_last_trim) all have work.
  sparse  64 splats of sigma ~ 1 px and opacity 0.3 .. 0.95 that leave tile (1, 0) empty, with culled ones (behind the
          camera, far off screen) and visible ones that no pixel composites (opacity below 1/255, or a centre so far
          outside the frame that only the tail of the splat reaches it).

walk() replays the oracle's compositing decisions in float64 to say WHERE in its tile list each pixel stops and which list
entries some pixel composites; the CPU test holds its alpha image to the oracle's, so it cannot drift from it.
"""
import functools
import math

import torch

from oracle import gsplat_oracle as G
from tests.scenes import random_scene, small_pose

W, H = 40, 24
TW, TH = math.ceil(W / 16), math.ceil(H / 16)
BATCH = 256  # list entries the compositing kernels stage at a time
CAMERAS = ((0.5, 0.01, 1), (1.5, 0.02, 2), (3.0, 0.03, 3))  # small_pose(degrees, metres, seed) per camera
PADDED = {6: 8, 9: 16, 17: 32}  # channel counts that are padded, and to what
# the sparse scene's rows: N_PLAIN ordinary splats, then ...
N_PLAIN, N_FAINT, N_EDGE, N_BEHIND, N_OFF = 46, 6, 6, 3, 3
EMPTY_TILE = (1, 0)  # (tx, ty)


def viewmats(C):
    """float32 world-to-camera matrices [C,4,4] of the first C cameras."""
    return torch.stack([torch.linalg.inv(small_pose(a, t, seed=s, dtype=torch.float32)) for a, t, s in CAMERAS[:C]]
                       ).contiguous()


@functools.lru_cache(maxsize=None)
def deep_scene(N=1200):
    return random_scene(N, W, H, seed=5, sigma_px=2.5, aniso=True, opacity=(0.02, 0.3), dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def sparse_scene():
    """float32 inputs like random_scene()'s, and the index sets "faint", "edge" (visible, composited by no pixel) and
    "culled" (radii 0).  Built on screen for the identity camera; the first camera of CAMERAS moves it by a fraction of a
    pixel."""
    g = torch.Generator().manual_seed(23)
    f64 = torch.float64
    fx, cx, cy = 0.5 * W, (W - 1) / 2.0, (H - 1) / 2.0
    rnd = lambda n: torch.rand(n, generator=g, dtype=f64)  # noqa: E731
    n_vis = N_PLAIN + N_FAINT
    # centres at least 7 px from the empty tile (x 16 .. 32, y 0 .. 16): the radius of these splats stays below 6
    u, v = [], []
    while len(u) < n_vis:
        a, b = float(rnd(1)) * W, float(rnd(1)) * H
        if not (16 - 7 < a < 32 + 7 and b < 16 + 7):
            u.append(a)
            v.append(b)
    u, v = torch.tensor(u, dtype=f64), torch.tensor(v, dtype=f64)
    # edge: 4.3 px left of the frame in the lower tile row, narrow in x: radius 5 reaches the frame, alpha at the first
    # pixel column stays far below 1/255
    u = torch.cat([u, torch.full((N_EDGE,), -4.3, dtype=f64), torch.tensor([20.0, 5.0, 30.0], dtype=f64),
                   torch.tensor([-60.0, 120.0, 20.0], dtype=f64)])
    v = torch.cat([v, 17.0 + 6.0 * rnd(N_EDGE), torch.tensor([8.0, 12.0, 20.0], dtype=f64),
                   torch.tensor([10.0, 12.0, -70.0], dtype=f64)])
    N = u.numel()
    z = 1.0 + 4.0 * rnd(N)
    z[n_vis + N_EDGE:n_vis + N_EDGE + N_BEHIND] = torch.tensor([-2.0, -0.5, 0.004], dtype=f64)  # behind / before near
    means = torch.stack([(u - cx) / fx * z, (v - cy) / fx * z, z], -1)
    quats = torch.randn(N, 4, generator=g, dtype=f64)
    scales = (1.0 * z.abs() / fx)[:, None] * (0.5 + rnd(3 * N).reshape(N, 3))
    edge = torch.arange(n_vis, n_vis + N_EDGE)
    quats[edge] = torch.tensor([1.0, 0, 0, 0], dtype=f64)
    scales[edge] = (z[edge] / fx)[:, None] * torch.tensor([0.9, 1.5, 0.2], dtype=f64)  # (thin along the ray as well)
    opac = 0.3 + 0.65 * rnd(N)
    faint = torch.arange(N_PLAIN, n_vis)
    opac[faint] = 0.0005 + 0.002 * rnd(N_FAINT)  # below 1/255 = 0.0039
    rgbs = rnd(3 * N).reshape(N, 3)
    K = torch.tensor([[fx, 0, cx], [0, fx, cy], [0, 0, 1]], dtype=f64)
    f32 = lambda t: t.float().contiguous()  # noqa: E731
    return dict(means=f32(means), quats=f32(quats), scales=f32(scales), opacities=f32(opac), rgbs=f32(rgbs), K=f32(K), W=W,
                H=H, faint=faint, edge=edge, culled=torch.arange(n_vis + N_EDGE, N))


SCENES = {"deep": deep_scene, "sparse": sparse_scene}


@functools.lru_cache(maxsize=None)
def stage_inputs(scene, C, D, N=None):
    """Inputs of rasterize_to_pixels for the first C cameras, as tests/test_gpu_parity.py's _stage_inputs makes them: the
    oracle's float32 projection and binning of the scene; colours [C,N,D] uniform in 0 .. 1 with the depth as the last
    channel, a background [C,D].  All float32 (ids: int32 / int64), on the host."""
    sc = SCENES[scene]() if N is None else SCENES[scene](N)
    Vs = viewmats(C)
    Ks = sc["K"][None].repeat(C, 1, 1)
    radii, m2, depths, conics, _ = G.fully_fused_projection(sc["means"], sc["quats"], sc["scales"], Vs, Ks, W, H)
    _, ids, flat = G.isect_tiles(m2, radii, depths, 16, TW, TH)
    offsets = G.isect_offset_encode(ids, C, TW, TH)
    gen = torch.Generator().manual_seed(100 * D + C)
    n = sc["means"].shape[0]
    colors = torch.rand(C, n, D, generator=gen)
    colors[..., -1] = depths
    backgrounds = torch.rand(C, D, generator=gen)
    return dict(means2d=m2.contiguous(), conics=conics.contiguous(), colors=colors.contiguous(),
                opacities=sc["opacities"][None].repeat(C, 1).contiguous(), offsets=offsets, flatten_ids=flat, radii=radii,
                backgrounds=backgrounds, C=C, N=n, D=D)


def walk(means2d, conics, opacities, offsets, flatten_ids):
    """The decisions of G.rasterize_to_pixels on these inputs, in float64, with G's constants.  Returns a dict of
    lengths [C,TH,TW] (tile list lengths), last_pos [C,H,W] (position within its tile's list of the last entry the pixel
    composites, -1: none), stopped [C,H,W] (the pixel met an entry that would have taken T to T_STOP or below),
    alphas [C,H,W], and per row of the flattened [C*N] arrays: composited (by some pixel), late (... at list position
    BATCH or later) and amax (the largest alpha the row has at any pixel of a tile that lists it; -1: in no list)."""
    C, N = opacities.shape
    m2, con, opa = means2d.double().reshape(C * N, 2), conics.double().reshape(C * N, 3), opacities.double().reshape(C * N)
    fid = flatten_ids.to(torch.int64)
    offs = offsets.reshape(-1).tolist() + [fid.numel()]
    out = dict(lengths=torch.zeros(C, TH, TW, dtype=torch.int64), last_pos=torch.full((C, H, W), -1, dtype=torch.int64),
               stopped=torch.zeros(C, H, W, dtype=torch.bool), alphas=torch.zeros(C, H, W, dtype=torch.float64),
               composited=torch.zeros(C * N, dtype=torch.bool), late=torch.zeros(C * N, dtype=torch.bool),
               amax=torch.full((C * N,), -1.0, dtype=torch.float64))
    for c in range(C):
        for ty in range(TH):
            y0, y1 = 16 * ty, min(16 * ty + 16, H)
            for tx in range(TW):
                x0, x1 = 16 * tx, min(16 * tx + 16, W)
                t = (c * TH + ty) * TW + tx
                s, e = offs[t], offs[t + 1]
                out["lengths"][c, ty, tx] = e - s
                if e <= s:
                    continue
                g = fid[s:e]
                py, px = torch.meshgrid(torch.arange(y0, y1, dtype=torch.float64) + 0.5,
                                        torch.arange(x0, x1, dtype=torch.float64) + 0.5, indexing="ij")
                dx, dy = m2[g, 0][None] - px.reshape(-1, 1), m2[g, 1][None] - py.reshape(-1, 1)
                cg = con[g]
                sigma = 0.5 * (cg[:, 0] * dx * dx + cg[:, 2] * dy * dy) + cg[:, 1] * dx * dy
                alpha = torch.clamp(opa[g][None] * torch.exp(-sigma), max=G.ALPHA_MAX)
                valid = (sigma >= 0) & (alpha >= G.ALPHA_MIN)
                a_eff = torch.where(valid, alpha, torch.zeros_like(alpha))
                incl = valid & (torch.cumprod(1 - a_eff, dim=1) > G.T_STOP)
                pos = torch.arange(e - s)
                shape = (y1 - y0, x1 - x0)
                out["last_pos"][c, y0:y1, x0:x1] = torch.where(incl, pos[None], -1).amax(1).reshape(shape)
                out["stopped"][c, y0:y1, x0:x1] = (valid & ~incl).any(1).reshape(shape)
                out["alphas"][c, y0:y1, x0:x1] = (1 - torch.where(incl, 1 - a_eff, torch.ones_like(a_eff)).prod(1)
                                                  ).reshape(shape)
                hit = incl.any(0)
                out["composited"][g[hit]] = True
                out["late"][g[hit & (pos >= BATCH)]] = True
                out["amax"][g] = torch.maximum(out["amax"][g], alpha.amax(0))  # (a tile lists a row once)
    return out


def tile_groups(means2d, radii):
    """The visible rows of the flattened [C*N] arrays, grouped by camera and by the tile that holds their centre (centres
    outside the frame: the nearest tile): what roll_within() rolls."""
    C, N = radii.shape
    m = means2d.reshape(C * N, 2)
    tx = (m[:, 0] / 16).floor().clamp(0, TW - 1).long()
    ty = (m[:, 1] / 16).floor().clamp(0, TH - 1).long()
    key = (torch.arange(C * N) // N) * (TW * TH) + ty * TW + tx
    vis = radii.reshape(-1) > 0
    return [((key == k) & vis).nonzero()[:, 0] for k in range(C * TW * TH) if int(((key == k) & vis).sum()) > 1]


def flat_rows(grads):
    """name -> [C,N,...] as name -> [C*N,...] (tests/grad_paths.py's compare_grads counts rows)."""
    return {k: t.reshape((-1,) + tuple(t.shape[2:])) for k, t in grads.items()}


# ---- rasterization() end to end -----------------------------------------------------------------------------------------
E2E_CASES = {  # name: cameras, feature channels (None: SH), render mode, background, antialiased, per-camera colours
    "c3-33ch": dict(C=3, feat=32, mode="RGB+ED", bg=True, aa=False, per_cam=False),
    "c2-16ch-antialiased": dict(C=2, feat=15, mode="RGB+D", bg=True, aa=True, per_cam=False),
    "c3-sh-per-camera": dict(C=3, feat=None, mode="RGB+ED", bg=True, aa=False, per_cam=True),
    "c2-rgb4-per-camera": dict(C=2, feat=4, mode="RGB", bg=False, aa=False, per_cam=True),
    "c1-2ch": dict(C=1, feat=1, mode="RGB+D", bg=False, aa=False, per_cam=False),
}
SH_DEGREE, SH_BANDS = 2, 16  # coefficients [C,N,16,3] of which degree 2 reads nine bands
E2E_NAMES = ("means", "quats", "scales", "opacities", "colors")


@functools.lru_cache(maxsize=None)
def e2e_inputs(name, scene="deep"):
    """float32 inputs of rasterization() for a case, on the host: the scene's Gaussians, colours / SH coefficients,
    viewmats, Ks, backgrounds (or None) and the keyword arguments both sides get."""
    case = E2E_CASES[name]
    sc = SCENES[scene]()
    C, n = case["C"], sc["means"].shape[0]
    gen = torch.Generator().manual_seed(31)
    lead = (C, n) if case["per_cam"] else (n,)
    if case["feat"] is None:
        colors = 0.3 * torch.randn(*lead, SH_BANDS, 3, generator=gen)
        n_bg = 3
    else:
        colors = torch.rand(*lead, case["feat"], generator=gen)
        n_bg = case["feat"]
    bg = torch.rand(C, n_bg, generator=gen) if case["bg"] else None
    ins = {k: sc[k] for k in ("means", "quats", "scales", "opacities")}
    ins.update(colors=colors, viewmats=viewmats(C), backgrounds=bg)
    kw = dict(width=W, height=H, sh_degree=SH_DEGREE if case["feat"] is None else None, render_mode=case["mode"],
              rasterize_mode="antialiased" if case["aa"] else "classic")
    return ins, sc["K"][None].repeat(C, 1, 1), kw


def oracle_e2e(ins, Ks, kw, dtype=torch.float64):
    """G.rasterization on the inputs in ``dtype``: (leaves, render, alphas, meta); the leaves require a gradient."""
    leaves = {k: t.to(dtype).clone().requires_grad_() for k, t in ins.items() if t is not None}
    r, a, meta = G.rasterization(leaves["means"], leaves["quats"], leaves["scales"], leaves["opacities"], leaves["colors"],
                                 leaves["viewmats"], Ks.to(dtype), backgrounds=leaves.get("backgrounds"), **kw)
    return leaves, r, a, meta


def oracle_grads(leaves, outputs, upstream):
    """name -> gradient of sum(output * upstream) over the outputs (zeros where the oracle has none)."""
    names = list(leaves)
    gs = torch.autograd.grad(list(outputs), [leaves[k] for k in names],
                             grad_outputs=[u.to(o.dtype) for o, u in zip(outputs, upstream)], retain_graph=True,
                             allow_unused=True)
    return {k: (t if t is not None else torch.zeros_like(leaves[k])) for k, t in zip(names, gs)}


def upstream(shape_c, shape_a, ok, seed=21):
    """Random upstream gradients (float64) of render and alphas, zero on the pixels where ``ok`` [C,H,W] is False."""
    gen = torch.Generator().manual_seed(seed)
    v = torch.randn(shape_c, generator=gen, dtype=torch.float64) * ok[..., None]
    va = torch.randn(shape_a, generator=gen, dtype=torch.float64) * ok[..., None]
    return v, va
