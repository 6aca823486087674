"""rasterization(absgrad=True) on the MI355X: means2d.grad and means2d.absgrad against per-pixel float64 gradients of
the oracle's stages, the invariants of an absolute sum, nothing else moving, and the full-size frames (R, the pile)."""
import math

import pytest
import torch

import gsplatloc_amd as A
from oracle import gsplat_oracle as G
from tests.scenes import random_scene, small_pose

pytestmark = pytest.mark.gpu

W, H = 32, 24  # 2 x 2 tiles, the second tile row half outside the image
N = 300
_X = {"RGB": 3, "D": 1, "ED": 1, "RGB+D": 4, "RGB+ED": 4}


def _scene(C=1, deg=None, seed=42, features=None):
    """``features``: that many feature channels per Gaussian in place of RGB (with deg=None)."""
    sc = random_scene(N, W, H, seed=seed, sigma_px=1.5, dtype=torch.float64, aniso=True, opacity=(0.3, 1.0))
    sc["means"][:4, 2] = -1.0  # behind the camera: radii 0
    g = torch.Generator().manual_seed(seed + 1)
    if features is not None:
        assert deg is None
        sc["colors"] = torch.rand(N, features, generator=g, dtype=torch.float64)
    elif deg is None:
        sc["colors"] = sc["rgbs"]
    else:
        sc["colors"] = 0.5 * torch.randn(N, (deg + 1) ** 2, 3, generator=g, dtype=torch.float64)
    sc["viewmats"] = torch.stack([torch.linalg.inv(small_pose(0.5, 0.01, seed=7 + 4 * c)) for c in range(C)])
    sc["Ks"] = sc["K"][None].repeat(C, 1, 1)
    return sc


def _upstream(C, mode, seed=3, channels=None):
    """``channels``: of the render, where the colours are feature vectors (default: the mode's with RGB)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(C, H, W, _X[mode] if channels is None else channels, generator=g, dtype=torch.float64),
            torch.randn(C, H, W, 1, generator=g, dtype=torch.float64))


def _oracle(sc, mode, deg, aa=False, bg=None, v=None, va=None):
    """float64 grad and absgrad of means2d [C,N,2]: one backward per pixel of L_p through the oracle's compositing."""
    C = sc["viewmats"].shape[0]
    radii, m2, depths, conics, comps = G.fully_fused_projection(
        sc["means"], sc["quats"], sc["scales"], sc["viewmats"], sc["Ks"], W, H, 0.3, 0.01, 1e10, 0.0, aa)
    opac = sc["opacities"][None].expand(C, -1)
    if comps is not None:
        opac = opac * comps
    if deg is None:
        cols = sc["colors"][None].expand(C, -1, -1)
    else:
        c2w = torch.linalg.inv(sc["viewmats"])
        dirs = sc["means"][None] - c2w[:, None, :3, 3]
        cols = G.spherical_harmonics(deg, dirs, sc["colors"][None].expand(C, -1, -1, -1), masks=radii > 0)
        cols = torch.clamp_min(cols + 0.5, 0.0)
    if mode in ("D", "ED"):
        cols = depths[..., None]
    elif mode != "RGB":
        cols = torch.cat([cols, depths[..., None]], dim=-1)
    if bg is not None and mode != "RGB":
        bg = torch.cat([bg, torch.zeros(C, 1, dtype=bg.dtype)], dim=-1)
    tw, th = math.ceil(W / 16), math.ceil(H / 16)
    _, isect_ids, flatten_ids = G.isect_tiles(m2, radii, depths, 16, tw, th)
    offsets = G.isect_offset_encode(isect_ids, C, tw, th)
    leaf = m2.detach().clone().requires_grad_()
    rc, ra = G.rasterize_to_pixels(leaf, conics.detach(), cols.detach(), opac.detach(), W, H, 16, offsets, flatten_ids,
                                   bg)
    if mode in ("ED", "RGB+ED"):
        rc = torch.cat([rc[..., :-1], rc[..., -1:] / ra.clamp(min=1e-10)], dim=-1)
    L = (rc * v).sum(-1) + (ra * va).sum(-1)  # [C,H,W]
    grad = torch.zeros(C, N, 2, dtype=torch.float64)
    absg = torch.zeros(C, N, 2, dtype=torch.float64)
    for c in range(C):
        for i in range(H):
            for j in range(W):
                if not L[c, i, j].requires_grad:
                    continue
                (gp,) = torch.autograd.grad(L[c, i, j], leaf, retain_graph=True)
                grad += gp
                absg += gp.abs()
    return grad, absg, radii


def _ours(sc, mode, deg, aa=False, bg=None, v=None, va=None, absgrad=True):
    C = sc["viewmats"].shape[0]
    dev = "cuda"
    f = lambda t: t.float().to(dev)  # noqa: E731
    ins = {k: f(sc[k]).requires_grad_() for k in ("means", "quats", "scales", "opacities", "colors", "viewmats")}
    r, a, info = A.rasterization(ins["means"], ins["quats"], ins["scales"], ins["opacities"], ins["colors"],
                                 ins["viewmats"], f(sc["Ks"]), W, H, sh_degree=deg, packed=False, absgrad=absgrad,
                                 render_mode=mode, backgrounds=None if bg is None else f(bg),
                                 rasterize_mode="antialiased" if aa else "classic")
    if absgrad:
        info["means2d"].retain_grad()
    ((r * f(v)).sum() + (a * f(va)).sum()).backward()
    torch.cuda.synchronize()
    return r, a, info, ins


def _agree(ours, ref, what, tol=1e-4, frac=0.002):
    """Per Gaussian, within tol of the largest reference value; ceil(frac) outliers for pixels on a threshold."""
    ours, ref = ours.detach().double().cpu(), ref.detach().double().cpu()
    assert torch.isfinite(ours).all(), what
    scale = float(ref.abs().max())
    assert scale > 0, what
    bad = ((ours - ref).abs().amax(-1) > tol * scale)
    n_bad = int(bad.sum())
    assert n_bad <= math.ceil(frac * bad.numel()), (what, n_bad, float((ours - ref).abs().max()) / scale)


CASES = [  # (path, mode, sh degree, antialiased, cameras, background)
    ("fused", "RGB", None, False, 1, False),
    ("fused", "D", None, False, 1, False),
    ("fused", "ED", None, False, 1, False),
    ("fused", "RGB+D", 3, False, 1, False),
    ("fused", "RGB+ED", 0, False, 1, False),
    ("fused", "RGB+ED", 3, True, 1, False),
    ("staged", "RGB+ED", 1, False, 2, False),
    ("staged", "RGB", None, False, 1, True),
    ("staged", "RGB+D", 0, True, 1, True),
]


@pytest.mark.parametrize("path,mode,deg,aa,C,with_bg", CASES)
def test_absgrad_and_grad_match_the_float64_oracle(path, mode, deg, aa, C, with_bg, monkeypatch):
    monkeypatch.setenv("GSLOC_DROPIN_CACHE", "0")
    sc = _scene(C, deg)
    v, va = _upstream(C, mode)
    bg = torch.rand(C, 3, generator=torch.Generator().manual_seed(9), dtype=torch.float64) if with_bg else None
    ref_grad, ref_abs, radii = _oracle(sc, mode, deg, aa, bg, v, va)
    r, a, info, _ = _ours(sc, mode, deg, aa, bg, v, va)
    m2 = info["means2d"]
    assert m2.shape == (C, N, 2) and m2.absgrad.shape == (C, N, 2) and m2.absgrad.dtype == torch.float32
    _agree(m2.absgrad, ref_abs, f"{path} {mode} absgrad")
    _agree(m2.grad, ref_grad, f"{path} {mode} grad")
    assert float(m2.absgrad[(radii == 0).cuda()].abs().max()) == 0.0


# the staged walk at the widths only feature vectors reach: k_absgrad<8>, <16>, <32> (features + the depth channel)
WIDE_CASES = [(7, 1, True), (15, 2, False), (31, 1, False)]  # (features, cameras, background)


@pytest.mark.parametrize("features,C,with_bg", WIDE_CASES)
def test_staged_absgrad_at_the_wide_widths(features, C, with_bg, monkeypatch):
    monkeypatch.setenv("GSLOC_DROPIN_CACHE", "0")
    monkeypatch.setenv("GSLOC_DISABLE_FUSED", "1")
    mode = "RGB+D"
    sc = _scene(C, None, features=features)
    v, va = _upstream(C, mode, channels=features + 1)
    bg = torch.rand(C, features, generator=torch.Generator().manual_seed(9), dtype=torch.float64) if with_bg else None
    ref_grad, ref_abs, radii = _oracle(sc, mode, None, False, bg, v, va)
    r, a, info, _ = _ours(sc, mode, None, False, bg, v, va)
    assert r.shape == (C, H, W, features + 1) and "Q0" not in info
    m2 = info["means2d"]
    assert m2.shape == (C, N, 2) and m2.absgrad.shape == (C, N, 2) and m2.absgrad.dtype == torch.float32
    _agree(m2.absgrad, ref_abs, f"staged {features + 1} channels absgrad")
    _agree(m2.grad, ref_grad, f"staged {features + 1} channels grad")
    assert float(m2.absgrad[(radii == 0).cuda()].abs().max()) == 0.0


def _check_invariants(sc, mode, deg, bg, v, va, tag):
    _, _, info, _ = _ours(sc, mode, deg, bg=bg, v=v, va=va)
    ab, gr = info["means2d"].absgrad.double(), info["means2d"].grad.double()
    scale = float(ab.max())
    assert scale > 0 and torch.isfinite(ab).all() and torch.isfinite(gr).all(), tag
    assert bool((ab >= gr.abs() - 1e-5 * scale).all()), (tag, float((gr.abs() - ab).max()) / scale)
    assert float(ab[info["radii"] == 0].abs().max()) == 0.0, tag
    # the upstream scaled by -3: absgrad scaled by 3
    _, _, info3, _ = _ours(sc, mode, deg, bg=bg, v=-3 * v, va=-3 * va)
    err = float((info3["means2d"].absgrad.double() - 3 * ab).abs().max()) / (3 * scale)
    assert err < 1e-5, (tag, err)
    # one pixel of upstream: nothing to cancel, absgrad = |grad|
    v1, va1 = torch.zeros_like(v), torch.zeros_like(va)
    v1[:, H // 2, W // 2 + 1] = v[:, H // 2, W // 2 + 1]
    va1[:, H // 2, W // 2 + 1] = va[:, H // 2, W // 2 + 1]
    _, _, info1, _ = _ours(sc, mode, deg, bg=bg, v=v1, va=va1)
    ab1, gr1 = info1["means2d"].absgrad.double(), info1["means2d"].grad.double()
    assert float(ab1.max()) > 0, tag
    assert float((ab1 - gr1.abs()).abs().max()) <= 1e-4 * float(ab1.max()), tag
    return info


@pytest.mark.parametrize("path,mode,deg,C,with_bg", [("fused", "RGB+ED", 1, 1, False), ("fused", "D", None, 1, False),
                                                     ("staged", "RGB+ED", 1, 2, False),
                                                     ("staged", "RGB", None, 1, True)])
def test_absgrad_invariants(path, mode, deg, C, with_bg, monkeypatch):
    monkeypatch.setenv("GSLOC_DROPIN_CACHE", "0")
    sc = _scene(C, deg, seed=5)
    v, va = _upstream(C, mode, seed=4)
    bg = torch.rand(C, 3, generator=torch.Generator().manual_seed(9), dtype=torch.float64) if with_bg else None
    info = _check_invariants(sc, mode, deg, bg, v, va, path)
    if path == "fused":  # .grad of the fused nodes = the staged operators' v_means2d
        monkeypatch.setenv("GSLOC_DISABLE_FUSED", "1")
        _, _, info_s, _ = _ours(sc, mode, deg, v=v, va=va)
        g_f, g_s = info["means2d"].grad.double(), info_s["means2d"].grad.double()
        assert float((g_f - g_s).abs().max()) <= 1e-4 * float(g_s.abs().max())
        _agree(info["means2d"].absgrad, info_s["means2d"].absgrad, "fused vs staged absgrad")


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


@pytest.mark.parametrize("path,mode,deg,C", [("fused", "RGB+ED", 1, 1), ("fused", "RGB", None, 1),
                                             ("staged", "RGB+ED", 1, 2)])
def test_absgrad_moves_nothing_else(path, mode, deg, C, monkeypatch):
    monkeypatch.setenv("GSLOC_DROPIN_CACHE", "0")
    sc = _scene(C, deg, seed=8)
    v, va = _upstream(C, mode, seed=6)
    r1, a1, info1, ins1 = _ours(sc, mode, deg, v=v, va=va, absgrad=True)
    r0, a0, info0, ins0 = _ours(sc, mode, deg, v=v, va=va, absgrad=False)
    assert torch.equal(r1, r0) and torch.equal(a1, a0)
    assert not hasattr(info0["means2d"], "absgrad")
    for k in ins0:
        assert _rel(ins1[k].grad, ins0[k].grad) < 1e-5, k
    with torch.no_grad():  # accepted, nothing attached
        sc32 = {k: sc[k].float().cuda() for k in ("means", "quats", "scales", "opacities", "colors", "viewmats", "Ks")}
        r2, _, info2 = A.rasterization(sc32["means"], sc32["quats"], sc32["scales"], sc32["opacities"], sc32["colors"],
                                       sc32["viewmats"], sc32["Ks"], W, H, sh_degree=deg, render_mode=mode,
                                       absgrad=True)
    assert torch.equal(r2, r0.detach()) and not hasattr(info2["means2d"], "absgrad")


def _full_size(which):
    from gsplatloc_amd import synthetic as S

    if which == "R":
        sc = S.random_scene(1_000_000, 1200, 680, device="cuda")
        Wf, Hf, V, K = 1200, 680, torch.linalg.inv(S.perturbed_pose()).cuda(), sc["K"]
    else:
        sc = S.depth_frame_scene(640, 480, stride=1, holes=True, device="cuda", pile=True)
        Wf, Hf, V, K = 640, 480, sc["viewmat"], sc["K"]
    g = torch.Generator().manual_seed(12)
    v = torch.randn(1, Hf, Wf, 4, generator=g).cuda()
    va = torch.randn(1, Hf, Wf, 1, generator=g).cuda()
    return sc, Wf, Hf, V[None].contiguous(), K[None].contiguous(), v, va


def _run_full(sc, Wf, Hf, V, K, v, va, absgrad=True):
    Vg = V.clone().requires_grad_()
    r, a, info = A.rasterization(sc["means"], sc["quats"], sc["scales"], sc["opacities"], sc["sh"], Vg, K, Wf, Hf,
                                 sh_degree=1, packed=False, absgrad=absgrad, render_mode="RGB+ED")
    if absgrad:
        info["means2d"].retain_grad()
    ((r * v).sum() + (a * va).sum()).backward()
    torch.cuda.synchronize()
    return r, info, Vg.grad


@pytest.mark.parametrize("which", ["R", "pile"])
def test_absgrad_at_full_size(which, monkeypatch):
    monkeypatch.setenv("GSLOC_DROPIN_CACHE", "0")
    sc, Wf, Hf, V, K, v, va = _full_size(which)
    r, info, _ = _run_full(sc, Wf, Hf, V, K, v, va)
    if which == "pile":  # the frame this case is for: one tile list above the long-list threshold of the cached path
        from gsplatloc_amd.context import LONG_MIN

        offs = info["isect_offsets"].reshape(-1).long()
        ends = torch.cat([offs[1:], offs.new_tensor([info["flatten_ids"].numel()])])
        assert int((ends - offs).max()) > LONG_MIN
    ab, gr = info["means2d"].absgrad.double(), info["means2d"].grad.double()
    scale = float(ab.max())
    assert scale > 0 and torch.isfinite(ab).all() and torch.isfinite(gr).all()
    assert bool((ab >= gr.abs() - 1e-5 * scale).all())
    assert float(ab[info["radii"] == 0].abs().max()) == 0.0
    _, info3, _ = _run_full(sc, Wf, Hf, V, K, -3 * v, -3 * va)
    assert float((info3["means2d"].absgrad.double() - 3 * ab).abs().max()) / (3 * scale) < 1e-5
    monkeypatch.setenv("GSLOC_DISABLE_FUSED", "1")
    _, info_s, _ = _run_full(sc, Wf, Hf, V, K, v, va)
    ab_s = info_s["means2d"].absgrad
    assert torch.isfinite(ab_s).all()
    _agree(info["means2d"].absgrad, ab_s, f"{which}: fused vs staged absgrad")
    _agree(info["means2d"].grad, info_s["means2d"].grad, f"{which}: fused vs staged grad")


def test_gsmodel_with_absgrad_config(monkeypatch):
    from gsplatloc_amd import synthetic as S
    from gsplatloc_amd.my_gsplat.model import GsConfig, GSModel

    monkeypatch.setenv("GSLOC_DROPIN_CACHE", "0")
    sc = S.random_scene(20_000, 320, 240, device="cuda")
    c2w = S.perturbed_pose().cuda()[None]
    v = torch.randn(1, 240, 320, 4, generator=torch.Generator().manual_seed(2)).cuda()
    out = {}
    for absgrad in (False, True):
        model = GSModel(sc["means"], sc["rgbs"], config=GsConfig(absgrad=absgrad), scales=sc["scales"])
        pose = c2w.clone().requires_grad_()
        colors, alphas, info = model(pose, sc["K"][None], 320, 240)
        ((colors * v).sum() + alphas.sum()).backward()
        torch.cuda.synchronize()
        out[absgrad] = (colors.detach(), pose.grad, info)
    assert _rel(out[True][0], out[False][0]) < 1e-5
    assert _rel(out[True][1], out[False][1]) < 1e-5
    ab = out[True][2]["means2d"].absgrad
    assert ab.shape == (1, 20_000, 2) and torch.isfinite(ab).all() and float(ab.max()) > 0
