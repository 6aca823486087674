"""The comparisons of the camera tests, written once for three kinds of "implementation" (test code only: every reference
value comes from oracle/gsplat_oracle.py, through tests/grad_paths.py and tests/staged_widths.py where they fit):

  the HIP kernels                     tests/test_gpu_cameras.py: every figure inside its bound;
  the float64 oracle at a WRONG camera  tests/test_cameras_cpu.py: every figure at least 100 x outside its bound;
  the oracle evaluated in float32     tests/test_cameras_cpu.py: every figure inside half its bound.

A figure is measured / bound, so 1.0 is the bound of the GPU test.  Where the GPU test allows a share of outliers (pixels
on a compositing threshold, Gaussians whose own alpha sits on 1/255) the figure is the factor by which the ELEMENT bound
would have to widen for the count to fit, i.e. the (allowed + 1)-th largest per-element ratio: above 1 exactly when the
GPU test's own check (agreeing_pixels, compare_grads / failing_subsets) fails.

The bounds are the project's: mostly_close's defaults (tests/test_gpu_parity.py), POSE_GRAD_TOL, IMAGE_RTOL / IMAGE_ATOL,
GRAD_RTOL / GRAD_ATOL / OUTLIER_FRAC, 2e-3 pixel outliers (test_rasterize_fwd_bwd), 0.999 radii agreement
(test_projection_fwd_bwd).
"""
import torch

from oracle import gsplat_oracle as G
from tests import staged_widths as S
from tests.grad_paths import GRAD_ATOL, GRAD_RTOL, MIN_SUBSET, OUTLIER_FRAC, compare_grads, oracle_render
from tests.parity import IMAGE_ATOL, IMAGE_RTOL, POSE_GRAD_TOL, agreeing_pixels, rel_inf
from tests.test_gpu_parity import mostly_close

CLOSE_RTOL, CLOSE_ATOL = mostly_close.__defaults__[:2]  # 1e-4, 1e-5
RADII_AGREE = 0.999     # radii equal except at ceil() borderlines
PIXEL_OUTLIERS = 2e-3   # pixels on a compositing threshold, per camera image
PROJ_OUT = ("means2d", "depths", "conics", "compensations")
PROJ_LEAVES = ("means", "quats", "scales", "viewmats")


def f64(t):
    return torch.as_tensor(t).detach().cpu().double()


def widening(ratios, allowed):
    """The factor by which a bound must widen for at most ``allowed`` of ``ratios`` (error / bound) to stay outside."""
    r = ratios.reshape(-1)
    if r.numel() <= allowed:
        return 0.0
    return float(torch.sort(r, descending=True)[0][allowed])


def allowed_in(n):
    """Outlier Gaussians compare_grads allows in a subset of n."""
    return int(OUTLIER_FRAC * n) if n >= MIN_SUBSET else 1


def gaussian_ratios(got, want):
    """[N]: per Gaussian the largest error / (GRAD_RTOL |o| + GRAD_ATOL max |o|) over the inputs in ``want`` and their
    elements -- compare_grads' element bound; above 1 where compare_grads marks the Gaussian."""
    out = None
    for nm, o in want.items():
        o = f64(o)
        o = o.reshape(o.shape[0], -1)
        g = f64(got[nm]).reshape(o.shape)
        err = (g - o).abs()
        bound = GRAD_RTOL * o.abs() + GRAD_ATOL * float(o.abs().max())
        r = torch.where(err > 0, err / bound.clamp(min=1e-300), torch.zeros_like(err)).amax(1)
        out = r if out is None else torch.maximum(out, r)
    return out


def gaussian_figures(got, want, subsets):
    """(figures, counts, worst): figures["v_gaussians <subset>"] over all the inputs in ``want`` and "v_<input> all" for
    each of them; compare_grads' counts and worst."""
    worst, counts, bad = compare_grads(got, want, subsets)
    ratios = gaussian_ratios(got, want)
    assert torch.equal(ratios > 1.0, bad), "gaussian_ratios and compare_grads disagree"
    figs = {f"v_gaussians {name}": widening(ratios[idx], allowed_in(int(idx.numel()))) for name, idx in subsets.items()}
    if "all" in subsets:  # and input by input
        idx = subsets["all"]
        for nm in want:
            figs[f"v_{nm} all"] = widening(gaussian_ratios(got, {nm: want[nm]})[idx], allowed_in(int(idx.numel())))
    return figs, counts, worst


class OracleRun:
    """Leaves (name -> tensor requiring a gradient), outputs of the oracle on them, and their vjp."""

    def __init__(self, leaves, outputs, **more):
        self.leaves, self.outputs = leaves, tuple(outputs)
        self.__dict__.update(more)

    def grads(self, *upstream):
        names = [k for k, t in self.leaves.items() if t.requires_grad]
        outs = [(o, u) for o, u in zip(self.outputs, upstream) if o is not None and o.requires_grad]
        if not outs:
            return {k: torch.zeros_like(self.leaves[k]).double() for k in names}
        gs = torch.autograd.grad([o for o, _ in outs], [self.leaves[k] for k in names],
                                 grad_outputs=[u.to(o.dtype) for o, u in outs], retain_graph=True, allow_unused=True)
        return {k: f64(t if t is not None else torch.zeros_like(self.leaves[k])) for k, t in zip(names, gs)}


# ---- projection ---------------------------------------------------------------------------------------------------------
def oracle_projection(sc, Ks=None, dtype=torch.float64):
    """G.fully_fused_projection with compensations on the float32 inputs of cameras.projection_case(), in ``dtype``."""
    leaves = {k: sc[k].to(dtype).clone().requires_grad_() for k in ("means", "quats", "scales")}
    leaves["viewmats"] = sc["Vs"].to(dtype).clone().requires_grad_()
    Ks = sc["Ks"] if Ks is None else Ks
    radii, m2, d, con, comp = G.fully_fused_projection(leaves["means"], leaves["quats"], leaves["scales"],
                                                       leaves["viewmats"], Ks.to(dtype), sc["W"], sc["H"],
                                                       calc_compensations=True, **sc["kw"])
    return OracleRun(leaves, (m2, d, con, comp), radii=radii)


def projection_upstream(want, keep, seed=11):
    """Random upstream gradients (float64) of means2d, depths, conics, compensations, zero off the rows ``keep`` [C,N]."""
    gen = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(o.shape, generator=gen, dtype=torch.float64) * keep.reshape(keep.shape + (1,) * (o.dim() - 2))
                 for o in want.outputs)


def projection_subsets(sc, radii):
    """The clamp groups, the rows exactly one camera sees, and all rows."""
    subsets = dict(sc["groups"])
    subsets["seen by one camera"] = ((radii > 0).sum(0) == 1).nonzero()[:, 0]
    subsets["all"] = torch.arange(sc["N"])
    return subsets


def projection_figures(sc, want, got, flip_aware=True):
    """``got``: radii [C,N], outputs (means2d, depths, conics, compensations) and grads(*upstream) -> name -> gradient, as
    OracleRun has them.  Values and upstream gradients on the rows both sides see with the same radius; with
    ``flip_aware=False`` (a wrong camera: few radii agree, and what is asked is how far the values move) on the rows both
    sides see.  Returns (figures, keep [C,N], counts, worst, the gradients of ``got``, those of ``want``)."""
    r_o, r_g = want.radii.cpu(), torch.as_tensor(got.radii).cpu()
    C = r_o.shape[0]
    agree = r_g == r_o
    keep = (agree if flip_aware else r_g > 0) & (r_o > 0)
    figs = {}
    for c in range(C):
        figs[f"radii [{c}]"] = (1.0 - agree[c].double().mean().item()) / (1.0 - RADII_AGREE)
        for nm, a, b in zip(PROJ_OUT, got.outputs, want.outputs):
            a, b = f64(a)[c][keep[c]], f64(b)[c][keep[c]]
            r = (a - b).abs() / (CLOSE_ATOL + CLOSE_RTOL * b.abs())
            figs[f"{nm} [{c}]"] = float(r.max()) if r.numel() else float("inf")  # (no row to compare: nothing is shown)
    ups = projection_upstream(want, keep)
    g_o, g_g = want.grads(*ups), got.grads(*ups)
    for c in range(C):
        figs[f"v_viewmats [{c}]"] = rel_inf(g_g["viewmats"][c, :3], g_o["viewmats"][c, :3]) / POSE_GRAD_TOL
    names = ("means", "quats", "scales")
    gf, counts, worst = gaussian_figures({k: g_g[k] for k in names}, {k: g_o[k] for k in names},
                                         projection_subsets(sc, r_o))
    figs.update(gf)
    return figs, keep, counts, worst, g_g, g_o


# ---- rasterization ------------------------------------------------------------------------------------------------------
def oracle_staged(ins, Ks, kw, dtype=torch.float64):
    """G.rasterization of a cameras.staged_case() (tests/staged_widths.py's oracle_e2e)."""
    leaves, r, a, meta = S.oracle_e2e(ins, Ks, kw, dtype=dtype)
    return OracleRun(leaves, (r, a), radii=meta["radii"])


def oracle_fused(sc, mode, K=None, dtype=torch.float64, half=False, antialiased=False):
    """oracle_render (tests/grad_paths.py) of a cameras.fused_case(), as [1,H,W,D] / [1,H,W,1]."""
    leaves = {k: sc[k].to(dtype).clone().requires_grad_() for k in ("means", "quats", "scales", "opacities")}
    rgb = mode.startswith("RGB")
    if rgb:
        leaves["colors"] = sc["sh"].to(dtype).clone().requires_grad_()
    leaves["viewmat"] = sc["V"].to(dtype).clone().requires_grad_()
    K = sc["K"] if K is None else K
    r, a = oracle_render(leaves["means"], leaves["quats"], leaves["scales"], leaves["opacities"], leaves.get("colors"),
                         leaves["viewmat"], K.to(dtype), sc["W"], sc["H"], mode, sh_degree=1 if rgb else None,
                         antialiased=antialiased, half=half, **sc["planes"])
    return OracleRun(leaves, (r[None], a[None]))


def pixel_ratios(render_a, alpha_a, render_b, alpha_b):
    """[...,H,W]: per pixel the largest |a - b| / (IMAGE_ATOL + IMAGE_RTOL |b|) over the channels and alpha --
    agreeing_pixels' rule; above 1 where agreeing_pixels says no."""
    ra, rb, aa, ab = f64(render_a), f64(render_b), f64(alpha_a), f64(alpha_b)
    aa, ab = aa.reshape(ra.shape[:-1] + (1,)), ab.reshape(rb.shape[:-1] + (1,))
    a, b = torch.cat([ra, aa], -1), torch.cat([rb, ab], -1)
    return ((a - b).abs() / (IMAGE_ATOL + IMAGE_RTOL * b.abs())).amax(-1)


def render_figures(want, got, subsets, pose="viewmats", rows=None, seed=21, flip_aware=True):
    """``want`` / ``got``: outputs (render [C,H,W,D], alphas [C,H,W,1]) and grads(v, va).  ``rows`` = (y0, y1): only these
    pixel rows are compared and carry an upstream gradient.  The upstream gradient is zero on the pixels that disagree
    (tests/parity.py); with ``flip_aware=False`` (a wrong camera: every pixel disagrees, and what is asked is how far the
    gradients move) it is not.  Returns (figures, flipped share per camera, counts, worst,
    the gradients of ``got``, those of ``want``)."""
    r_o, a_o = (f64(t) for t in want.outputs)
    r_g, a_g = (f64(t) for t in got.outputs)
    C, H, W = r_o.shape[:3]
    y0, y1 = (0, H) if rows is None else rows
    ok = agreeing_pixels(r_g, a_g, r_o, a_o)
    ratios = pixel_ratios(r_g, a_g, r_o, a_o)
    assert torch.equal(ratios <= 1.0, ok), "pixel_ratios and agreeing_pixels disagree"
    ok[:, :y0] = False
    ok[:, y1:] = False
    n_pix = (y1 - y0) * W
    figs, flipped = {}, []
    for c in range(C):
        flipped.append(1.0 - ok[c, y0:y1].double().mean().item())
        figs[f"pixels [{c}]"] = widening(ratios[c, y0:y1], int(PIXEL_OUTLIERS * n_pix))
    lit = ok if flip_aware else torch.ones_like(ok)
    lit[:, :y0] = False
    lit[:, y1:] = False
    v, va = S.upstream(r_o.shape, a_o.shape, lit, seed=seed)
    g_o, g_g = want.grads(v, va), got.grads(v, va)
    vo, vg = g_o[pose].reshape(C, 4, 4), f64(g_g[pose]).reshape(C, 4, 4)
    for c in range(C):
        figs[f"v_{pose} [{c}]"] = rel_inf(vg[c, :3], vo[c, :3]) / POSE_GRAD_TOL
    names = [k for k in ("means", "quats", "scales", "opacities", "colors") if k in g_o and float(g_o[k].abs().max()) > 0]
    gf, counts, worst = gaussian_figures({k: g_g[k] for k in names}, {k: g_o[k] for k in names}, subsets)
    figs.update(gf)
    if "backgrounds" in g_o:
        figs["v_backgrounds"] = rel_inf(g_g["backgrounds"], g_o["backgrounds"]) / POSE_GRAD_TOL
    return figs, flipped, counts, worst, g_g, g_o


def flipped_within_cap(flipped):
    return all(f <= PIXEL_OUTLIERS for f in flipped)


def staged_subsets(sc, radii):
    """The clamp groups, the rows exactly one camera sees, every row some camera sees."""
    subsets = dict(sc["groups"])
    subsets["seen by one camera"] = ((radii > 0).sum(0) == 1).nonzero()[:, 0]
    subsets["all"] = (radii > 0).any(0).nonzero()[:, 0]
    return subsets


def fused_subsets(sc):
    """The clamp groups (where the case has them) and all rows."""
    subsets = dict(sc["groups"])
    subsets["all"] = torch.arange(sc["N"])
    return subsets


# ---- wrong cameras ------------------------------------------------------------------------------------------------------
def exchange_focal(K, W, H):
    out = K.clone()
    out[..., 0, 0], out[..., 1, 1] = K[..., 1, 1], K[..., 0, 0]
    return out


def exchange_centre(K, W, H):
    out = K.clone()
    out[..., 0, 2], out[..., 1, 2] = K[..., 1, 2], K[..., 0, 2]
    return out


def image_centre(K, W, H):
    out = K.clone()
    out[..., 0, 2], out[..., 1, 2] = (W - 1) / 2.0, (H - 1) / 2.0
    return out


def first_camera(Ks, W, H):
    return Ks[:1].expand_as(Ks).clone()


MUTATIONS = {"fx-fy-exchanged": exchange_focal, "cx-cy-exchanged": exchange_centre, "principal-point-centred": image_centre,
             "camera-0-everywhere": first_camera}
