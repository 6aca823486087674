"""The reference stands and the inputs discriminate, for the cameras of tests/cameras.py (fx != fy, an off-centre
fractional principal point, a different K per camera).  Runs without a GPU; tests/test_gpu_cameras.py rests on it.

(a) the C oracle and the autograd oracle agree at these cameras (render, alphas, every gradient);
(b) the float64 oracle at a WRONG camera -- fx and fy exchanged, cx and cy exchanged, the principal point replaced by the
    image centre, every camera given camera 0's K -- is at least 100 x outside the bound the GPU test applies, for every
    quantity the GPU test compares, on the GPU test's own inputs.  A quantity that a mutation cannot move is listed by
    name (NOT_EVIDENCE_*) and is held to stay below 100, so the lists stay true;
(c) the oracle evaluated in float32 stays inside every cap of the GPU test on those inputs with a factor of two to spare.

Figures are measured / bound (tests/camera_checks.py); they are printed.
"""
import numpy as np
import pytest
import torch

from oracle import c_oracle as C
from oracle import gsplat_oracle as G
from tests import camera_checks as X
from tests import cameras as cam
from tests.scenes import random_scene, small_pose

FAR = 100.0   # (b): a wrong camera is at least this many bounds away
SPARE = 2.0   # (c): the float32 oracle keeps this factor to every cap


# ---- the inputs are what they say -----------------------------------------------------------------------------------------
def test_control_camera_gives_random_scene():
    W, H = 96, 64
    a = random_scene(300, W, H, seed=3, sigma_px=1.5, aniso=True, opacity=(0.2, 0.9))
    b = cam.camera_scene(300, W, H, cam.skewed_K(W, H, "control"), seed=3, sigma_px=1.5, aniso=True, opacity=(0.2, 0.9))
    for k in ("means", "quats", "opacities", "rgbs", "K"):
        assert torch.equal(a[k], b[k]), k
    assert torch.allclose(a["scales"], b["scales"], rtol=1e-15, atol=0)


@pytest.mark.parametrize("which", cam.CAMERAS)
@pytest.mark.parametrize("shape", [(96, 64), (100, 70)])
def test_clamp_rows_take_the_branches_they_name(which, shape):
    """In front of the identity camera the oracle's own clamp (persp_proj) acts on exactly the named axes, the large rows
    are visible and the three cull rows are culled."""
    W, H = shape
    K = cam.skewed_K(W, H, which)
    rows = cam.clamp_rows(K, W, H)
    assert K[0, 1] == 0 and sorted(rows["groups"]) == sorted(cam.CLAMP_GROUPS)
    n = cam.N_CLAMP
    m = rows["means"][:n]
    lim_x, lim_y = cam.clamp_limits(K, W, H)
    assert lim_x == G.FOV_LIM_FACTOR * 0.5 * W / float(K[0, 0]) and lim_y == G.FOV_LIM_FACTOR * 0.5 * H / float(K[1, 1])
    cov = torch.eye(3, dtype=torch.float64).repeat(n, 1, 1)
    _, c_here = G.persp_proj(m, cov, K, W, H)
    _, c_free = G.persp_proj(m, cov, K, W * 1000, H * 1000)  # (an image so wide that nothing clamps)
    x_cl = (c_here[:, 0, 0] - c_free[:, 0, 0]).abs() > 1e-9   # J's third column: -fx tx / z^2 in row 0, -fy ty / z^2 in row 1
    y_cl = (c_here[:, 1, 1] - c_free[:, 1, 1]).abs() > 1e-9
    g = rows["groups"]
    assert x_cl[g["x only"]].all() and not y_cl[g["x only"]].any()
    assert y_cl[g["y only"]].all() and not x_cl[g["y only"]].any()
    assert x_cl[g["both"]].all() and y_cl[g["both"]].all()
    assert not x_cl[g["neither"]].any() and not y_cl[g["neither"]].any()
    radii = G.fully_fused_projection(rows["means"], rows["quats"], rows["scales"], torch.eye(4, dtype=torch.float64)[None],
                                     K[None], W, H, **rows["kw"])[0][0]
    assert (radii[:n] > 0).all(), radii
    assert [int(radii[i]) for i in rows["culled"].values()] == [0, 0, 0]
    # without radius_clip the last row is seen: it is that cull, and no other, which removes it
    kw = dict(rows["kw"], radius_clip=0.0)
    r0 = G.fully_fused_projection(rows["means"], rows["quats"], rows["scales"], torch.eye(4, dtype=torch.float64)[None],
                                  K[None], W, H, **kw)[0][0]
    assert int(r0[rows["culled"]["below radius_clip"]]) > 0


def test_three_cameras_differ():
    Ks, Vs = cam.three_cameras(96, 64)
    assert Ks.shape == (3, 3, 3) and Vs.shape == (3, 4, 4)
    for a in range(3):
        for b in range(a + 1, 3):
            assert not torch.allclose(Ks[a], Ks[b]) and not torch.allclose(Vs[a], Vs[b])
    sc = cam.projection_case()
    radii = X.oracle_projection(sc).radii
    seen = (radii > 0).sum(1)
    assert len(set(seen.tolist())) == 3 and int(seen.min()) > 500, seen  # another visible set per camera
    subsets = X.projection_subsets(sc, radii)
    assert int(subsets["seen by one camera"].numel()) >= 100
    for name, rows in sc["culled"].items():  # each cull row is culled in every camera
        assert int(radii[:, rows].abs().max()) == 0, name


# ---- (a) the two oracles agree ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c_oracle():
    C.build()
    return C


@pytest.mark.parametrize("aa", [False, True], ids=["classic", "antialiased"])
@pytest.mark.parametrize("mode,sh", [("RGB+ED", 1), ("ED", None)])
@pytest.mark.parametrize("which", ["wide_x", "wide_y"])
def test_c_oracle_and_autograd_oracle_agree_at_a_skewed_camera(which, mode, sh, aa, c_oracle):
    """tests/test_c_oracle.py's bounds (1e-10 relative on the images, 1e-9 of the largest entry on every gradient) on
    camera_scene + clamp_rows; the C oracle takes one camera."""
    N, W, H = 400, 57, 41
    K = cam.skewed_K(W, H, which)
    sc = cam.camera_scene(N, W, H, K, seed=11, sigma_px=2.0, aniso=True, opacity=(0.2, 0.95))
    sc = cam.with_rows(sc, [cam.clamp_rows(K, W, H)])
    n = sc["N"]
    g = torch.Generator().manual_seed(5)
    rgb = mode.startswith("RGB")
    colors = 0.3 * torch.randn(n, 4, 3, generator=g, dtype=torch.float64) if rgb else torch.zeros(n, 3, dtype=torch.float64)
    V = torch.linalg.inv(small_pose(1.5, 0.05, seed=11))
    D = 4 if rgb else 1
    v_render = torch.randn(H, W, D, generator=g, dtype=torch.float64)
    v_alphas = torch.randn(H, W, generator=g, dtype=torch.float64)
    ins = [sc[k].clone().requires_grad_() for k in ("means", "quats", "scales", "opacities")]
    col, Vg = colors.clone().requires_grad_(), V.clone().requires_grad_()
    rc, ra, meta = G.rasterization(*ins, col, Vg[None], K[None], W, H, sh_degree=sh, render_mode=mode,
                                   rasterize_mode="antialiased" if aa else "classic", **cam.CLAMP_KW)
    ((rc[0] * v_render).sum() + (ra[0, ..., 0] * v_alphas).sum()).backward()
    radii = meta["radii"][0]
    assert int(radii[N:N + cam.N_CLAMP].gt(0).sum()) >= 8 and int(radii[N + cam.N_CLAMP:].abs().max()) == 0
    out = c_oracle.rasterization(sc["means"], sc["quats"], sc["scales"], sc["opacities"], colors, V, K, W, H,
                                 sh_degree=sh, render_mode=mode, v_render=v_render, v_alphas=v_alphas, antialiased=aa,
                                 threads=4, **cam.CLAMP_KW)
    assert out["n_isects"] == meta["flatten_ids"].numel() > N // 2
    np.testing.assert_allclose(out["render"], rc[0].detach().numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(out["alphas"], ra[0, ..., 0].detach().numpy(), rtol=1e-10, atol=1e-12)
    pairs = [("means", out["v_means"], ins[0].grad), ("quats", out["v_quats"], ins[1].grad),
             ("scales", out["v_scales"], ins[2].grad), ("opacities", out["v_opacities"], ins[3].grad),
             ("viewmat", out["v_viewmat"][:3], Vg.grad[:3])]
    if rgb:
        pairs.append(("colors", out["v_colors"], col.grad))
    for name, got, want in pairs:
        want = want.numpy()
        assert np.abs(got - want).max() <= 1e-9 * max(np.abs(want).max(), 1e-30), (which, name)


# ---- (b) a wrong camera is far outside every bound ------------------------------------------------------------------------
def _touched(Ks, wrong):
    return [c for c in range(Ks.shape[0]) if not torch.equal(Ks[c], wrong[c])]


def _judge(tag, figs, touched, not_evidence):
    """Every per-camera figure of a touched camera and every per-Gaussian figure over all rows (the inputs together and
    one by one): at least FAR, unless its kind is listed -- then below FAR."""
    lines, failures = [], []
    for name, x in figs.items():
        kind, _, c = name.partition(" [")
        if c:
            if int(c[:-1]) not in touched:
                continue
        elif not name.endswith(" all"):
            lines.append(f"    {name}: {x:.3g} (printed only)")
            continue
        listed = kind in not_evidence
        lines.append(f"    {name}: {x:.3g}" + (" (listed: no evidence)" if listed else ""))
        if listed != (x < FAR):
            failures.append((name, x, "listed as unmoved" if listed else "not moved"))
    print(f"[cameras] {tag}: measured / bound\n" + "\n".join(lines))
    assert not failures, (tag, failures)


# The projection operator alone reads cx and cy in one place, the centre: every other output and -- the upstream gradients
# being given -- every gradient is the same function of the inputs wherever the principal point is.  Only means2d can
# tell.  The camera-space depth reads no intrinsic at all.
_CENTRE_ONLY = ("radii", "depths", "conics", "compensations", "v_viewmats", "v_gaussians all", "v_means all", "v_quats all",
                "v_scales all")
NOT_EVIDENCE_PROJECTION = {
    "fx-fy-exchanged": ("depths",),
    "cx-cy-exchanged": _CENTRE_ONLY[1:],  # (exchanging 45 px for 35 px moves a fifth of the rows across the frame's border)
    "principal-point-centred": _CENTRE_ONLY,
    "camera-0-everywhere": ("depths",),
}
NOT_EVIDENCE_RENDER = {name: () for name in X.MUTATIONS}  # a render samples the pixel grid: every quantity moves


@pytest.mark.parametrize("mutation", list(X.MUTATIONS))
def test_a_wrong_camera_moves_the_projection(mutation):
    sc = cam.projection_case()
    want = X.oracle_projection(sc)
    wrong = X.MUTATIONS[mutation](sc["Ks"], sc["W"], sc["H"])
    figs, keep, _, _, _, _ = X.projection_figures(sc, want, X.oracle_projection(sc, Ks=wrong), flip_aware=False)
    assert int(keep.sum()) > 1000
    _judge(f"projection, {mutation}", figs, _touched(sc["Ks"], wrong), NOT_EVIDENCE_PROJECTION[mutation])


@pytest.mark.parametrize("mutation", list(X.MUTATIONS))
@pytest.mark.parametrize("name", ["sh2", "ed"])
def test_a_wrong_camera_moves_the_staged_render(name, mutation):
    ins, Ks, kw, sc = cam.staged_case(name)
    want = X.oracle_staged(ins, Ks, kw)
    wrong = X.MUTATIONS[mutation](Ks, kw["width"], kw["height"])
    subsets = {"all": (want.radii > 0).any(0).nonzero()[:, 0]}
    figs, _, _, _, _, _ = X.render_figures(want, X.oracle_staged(ins, wrong, kw), subsets, flip_aware=False)
    _judge(f"staged {name}, {mutation}", figs, _touched(Ks, wrong), NOT_EVIDENCE_RENDER[mutation])


@pytest.mark.parametrize("mutation", list(X.MUTATIONS)[:3])
@pytest.mark.parametrize("name", ["general-wide_x", "general-wide_y", "tiny-wide_x"])
def test_a_wrong_camera_moves_the_fused_render(name, mutation):
    sc = cam.fused_case(name)
    mode = cam.FUSED_CASES[name]["mode"]
    want = X.oracle_fused(sc, mode)
    wrong = X.MUTATIONS[mutation](sc["K"], sc["W"], sc["H"])
    figs, _, _, _, _, _ = X.render_figures(want, X.oracle_fused(sc, mode, K=wrong), {"all": torch.arange(sc["N"])},
                                        pose="viewmat", flip_aware=False)
    _judge(f"fused {name}, {mutation}", figs, [0], NOT_EVIDENCE_RENDER[mutation])


# ---- (c) the float32 oracle keeps a factor of two to every cap ----------------------------------------------------------
def _spare(tag, figs, counts, flipped=()):
    lines = [f"    {k}: margin {1.0 / x if x > 0 else float('inf'):.3g}" for k, x in figs.items()
             if not k.startswith(("pixels", "v_gaussians"))]
    lines += [f"    outlier Gaussians, {k}: {c[0]} of {c[1]} (allowed {c[2]})" for k, c in counts.items()]
    lines += [f"    flipped pixels [{c}]: {f:.2e} (cap {X.PIXEL_OUTLIERS:.0e})" for c, f in enumerate(flipped)]
    print(f"[cameras] float32 oracle, {tag}:\n" + "\n".join(lines))
    for k, x in figs.items():
        if not k.startswith(("pixels", "v_gaussians")):  # (those two are shares: counted below)
            assert SPARE * x <= 1.0, (tag, k, x)
    for k, (n_bad, n, allowed) in counts.items():
        assert SPARE * n_bad <= allowed, (tag, "outlier Gaussians", k, n_bad, n, allowed)
    for c, f in enumerate(flipped):
        assert SPARE * f <= X.PIXEL_OUTLIERS, (tag, "flipped pixels of camera", c, f)


def test_float32_oracle_projection_is_inside_the_caps():
    sc = cam.projection_case()
    figs, keep, counts, _, _, _ = X.projection_figures(sc, X.oracle_projection(sc),
                                                    X.oracle_projection(sc, dtype=torch.float32))
    assert int(keep.sum()) > 1000
    _spare("projection", figs, counts)


@pytest.mark.parametrize("name", list(cam.STAGED_CASES))
def test_float32_oracle_staged_render_is_inside_the_caps(name):
    ins, Ks, kw, sc = cam.staged_case(name)
    want = X.oracle_staged(ins, Ks, kw)
    figs, flipped, counts, _, _, _ = X.render_figures(want, X.oracle_staged(ins, Ks, kw, dtype=torch.float32),
                                                   X.staged_subsets(sc, want.radii))
    _spare(f"staged {name}", figs, counts, flipped)


@pytest.mark.parametrize("name", list(cam.FUSED_CASES))
def test_float32_oracle_fused_render_is_inside_the_caps(name):
    sc = cam.fused_case(name)
    case = cam.FUSED_CASES[name]
    kw = dict(half=case["ctx"].get("staging") == "fp16", antialiased=case["ctx"].get("antialiased", False))
    rows = case["ctx"].get("tile_rows")
    rows = None if rows is None else (16 * rows[0], min(16 * rows[1], sc["H"]))
    figs, flipped, counts, _, _, _ = X.render_figures(X.oracle_fused(sc, case["mode"], **kw),
                                                   X.oracle_fused(sc, case["mode"], dtype=torch.float32, **kw),
                                                   X.fused_subsets(sc), pose="viewmat", rows=rows)
    _spare(f"fused {name}", figs, counts, flipped)
