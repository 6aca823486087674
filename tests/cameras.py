"""Cameras with fx != fy and an off-centre, fractional principal point, and the scenes built for them (inputs only; no
oracle code).  tests/test_cameras_cpu.py shows that these inputs tell a wrong camera from the right one and that the
float32 oracle stays inside the caps on them; tests/test_gpu_cameras.py runs the kernels on them.

The projection reads four camera scalars per axis pair: fx / fy, cx / cy, the frustum clamp limits lim_x / lim_y
(1.3 * 0.5 * W / fx and 1.3 * 0.5 * H / fy) and the x / y clamp branches of the vjp.  With fx == fy and a centred
principal point an exchange of an x-term for a y-term gives the same bits; with the cameras below it does not.
"""
import functools

import torch

from tests.scenes import frustum_clamp_scene, small_pose

CAMERAS = ("wide_x", "wide_y", "control")
POSES = ((0.5, 0.01, 11), (2.0, 0.03, 12), (4.0, 0.05, 13))  # small_pose(degrees, metres, seed) of three_cameras()
FOV_LIM = 1.3  # gsplat clamps x/z and y/z to 1.3 tan(fov/2) in the EWA Jacobian
CLAMP_KW = dict(frustum_clamp_scene()["kw"])  # near_plane, far_plane, radius_clip of the clamp rows
CLAMP_GROUPS = ("x only", "y only", "both", "neither")
CULL_ROWS = ("behind", "beyond far", "below radius_clip")
N_CLAMP = 12  # rows of clamp_rows() in front of the three culled ones


def skewed_K(W, H, which, dtype=torch.float64):
    """The test cameras [3,3] (K[0,1] stays 0: gsplat and the kernels ignore skew)."""
    if which == "wide_x":
        fx, fy, cx, cy = 0.62 * W, 0.81 * W, W / 2.0 - 3.3, H / 2.0 + 2.6
    elif which == "wide_y":
        fx, fy, cx, cy = 0.84 * W, 0.60 * W, W / 2.0 + 4.7, H / 2.0 - 1.4
    elif which == "control":  # random_scene's own camera
        fx, fy, cx, cy = 0.5 * W, 0.5 * W, (W - 1) / 2.0, (H - 1) / 2.0
    else:
        raise ValueError(which)
    return torch.tensor([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=torch.float64).to(dtype)


def intrinsics(K):
    """fx, fy, cx, cy of a [3,3] matrix as Python floats."""
    return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])


def camera_scene(N, W, H, K, seed=42, sigma_px=1.0, aniso=False, opacity=None, dtype=torch.float64):
    """tests/scenes.py random_scene's recipe (same draws in the same order) with u, v uniform on the image OF THE GIVEN K:
    means = ((u - cx) / fx * z, (v - cy) / fy * z, z); scales sigma_px * z / sqrt(fx * fy).  Same dict keys."""
    g = torch.Generator().manual_seed(seed)
    f64 = torch.float64
    fx, fy, cx, cy = intrinsics(K.double())
    u = torch.rand(N, generator=g, dtype=f64) * W
    v = torch.rand(N, generator=g, dtype=f64) * H
    z = 1.0 + 4.0 * torch.rand(N, generator=g, dtype=f64)
    means = torch.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], -1)
    f = (fx * fy) ** 0.5
    if aniso:
        quats = torch.randn(N, 4, generator=g, dtype=f64)
        scales = (sigma_px * z / f)[:, None] * (0.5 + torch.rand(N, 3, generator=g, dtype=f64))
    else:
        quats = torch.tensor([1.0, 0, 0, 0], dtype=f64).repeat(N, 1)
        scales = (sigma_px * z / f)[:, None].repeat(1, 3)
    if opacity is None:
        opac = torch.ones(N, dtype=f64)
    else:
        opac = opacity[0] + (opacity[1] - opacity[0]) * torch.rand(N, generator=g, dtype=f64)
    rgbs = torch.rand(N, 3, generator=g, dtype=f64)
    return dict(means=means.to(dtype), quats=quats.to(dtype), scales=scales.to(dtype), opacities=opac.to(dtype),
                rgbs=rgbs.to(dtype), K=K.double().to(dtype), W=W, H=H)


def clamp_limits(K, W, H):
    """lim_x, lim_y: where the EWA Jacobian of this camera starts to clamp x/z and y/z."""
    fx, fy, _, _ = intrinsics(K)
    return FOV_LIM * 0.5 * W / fx, FOV_LIM * 0.5 * H / fy


def clamp_group(xz, yz, K, W, H):
    """Index into CLAMP_GROUPS per point from its camera-space x/z and y/z under camera K."""
    lim_x, lim_y = clamp_limits(K, W, H)
    cx, cy = xz.abs() > lim_x, yz.abs() > lim_y
    out = torch.full(xz.shape, 3, dtype=torch.int64)
    out[cx & ~cy] = 0
    out[~cx & cy] = 1
    out[cx & cy] = 2
    return out


def swapped(K):
    """K with fx and fy exchanged."""
    Ks = K.clone()
    Ks[0, 0], Ks[1, 1] = K[1, 1], K[0, 0]
    return Ks


def clamp_rows(K, W, H, seed=31, opacity=(0.05, 0.25), dtype=torch.float64):
    """Twelve large Gaussians in the style of frustum_clamp_scene, at depth 2 in front of the identity camera and placed
    relative to THIS K's limits: three clamped in x only, three in y only, three in both, three in neither (rows
    0 .. 11 in that order, at least 15 % of the limit away from it), then one behind the camera, one beyond far_plane and
    one below radius_clip (rows 12, 13, 14; CLAMP_KW).  Their opacities are low: they cover the frame.

    With fx != fy the limits of the camera with fx and fy exchanged differ on both axes, and a window of (x/z, y/z)
    belongs to another group there.  Only one of the two one-axis groups has such a window -- x only when fx > fy
    (x/z in (lim_x, lim_x'], y/z in (lim_y', lim_y]: y only under the exchanged camera), y only when fy > fx; the other
    one-axis group keeps its class whatever the exchange -- so that group holds two rows in the window, asserted here.
    Returns random_scene's keys and groups (name -> rows), culled (name -> row), kw."""
    K = K.double()
    g = torch.Generator().manual_seed(seed)
    f64 = torch.float64
    fx, fy, _, _ = intrinsics(K)
    lx, ly = clamp_limits(K, W, H)
    lxs, lys = clamp_limits(swapped(K), W, H)
    x_only = [(1.3, 0.2), (-1.25, -0.5), (1.2, -0.7)]
    y_only = [(0.1, -1.3), (-0.6, 1.25), (0.75, 1.2)]
    xz = [a * lx for a, _ in x_only] + [a * lx for a, _ in y_only]
    yz = [b * ly for _, b in x_only] + [b * ly for _, b in y_only]
    window = [] if fx == fy else ([1, 2] if fx > fy else [4, 5])  # x only -> y only, or y only -> x only
    for i, s in zip(window, (-1.0, 1.0)):
        xz[i], yz[i] = s * 0.5 * (lx + lxs), -s * 0.5 * (ly + lys)
    xz += [1.25 * lx, -1.35 * lx, -1.2 * lx, 0.1 * lx, -0.5 * lx, 0.7 * lx]
    yz += [-1.3 * ly, 1.2 * ly, -1.25 * ly, -0.2 * ly, 0.6 * ly, 0.75 * ly]
    xz, yz = torch.tensor(xz, dtype=f64), torch.tensor(yz, dtype=f64)
    want = torch.arange(N_CLAMP) // 3
    assert torch.equal(clamp_group(xz, yz, K, W, H), want)
    plain = torch.ones(N_CLAMP, dtype=torch.bool)
    plain[window] = False
    for s in (0.87, 1.15):  # the rows outside the window keep their group 13 % nearer and 15 % farther
        assert torch.equal(clamp_group(s * xz, s * yz, K, W, H)[plain], want[plain])
    if window:
        there = clamp_group(xz, yz, swapped(K), W, H)
        assert there[window].tolist() == [1 - int(want[window[0]])] * 2, "window rows do not change their group"
    z = torch.full((N_CLAMP,), 2.0, dtype=f64)
    means = torch.stack([xz * z, yz * z, z], -1)
    sigma = 0.28 * W * 2.0 / (fx * fy) ** 0.5  # ~ 0.28 W pixels wide: reaches the frame from 0.35 W outside it
    scales = sigma * (0.7 + 0.6 * torch.rand(N_CLAMP, 3, generator=g, dtype=f64))
    means = torch.cat([means, torch.tensor([[0.0, 0.0, -0.5], [0.1, 0.0, 50.0], [0.0, 0.1, 2.0]], dtype=f64)])
    scales = torch.cat([scales, torch.tensor([[0.1] * 3, [0.1] * 3, [1e-3] * 3], dtype=f64)])
    n = means.shape[0]
    quats = torch.randn(n, 4, generator=g, dtype=f64)
    opac = opacity[0] + (opacity[1] - opacity[0]) * torch.rand(n, generator=g, dtype=f64)
    rgbs = torch.rand(n, 3, generator=g, dtype=f64)
    t = lambda x: x.to(dtype)  # noqa: E731
    return dict(means=t(means), quats=t(quats), scales=t(scales), opacities=t(opac), rgbs=t(rgbs), K=t(K), W=W, H=H,
                groups={name: torch.arange(3 * i, 3 * i + 3) for i, name in enumerate(CLAMP_GROUPS)},
                culled={name: N_CLAMP + i for i, name in enumerate(CULL_ROWS)}, kw=dict(CLAMP_KW))


def three_cameras(W, H, dtype=torch.float64):
    """Ks [3,3,3] = (wide_x, wide_y, control) and three world-to-camera matrices [3,4,4] of different seeds and sizes."""
    Ks = torch.stack([skewed_K(W, H, which) for which in CAMERAS])
    Vs = torch.stack([torch.linalg.inv(small_pose(a, t, seed=s)) for a, t, s in POSES])
    return Ks.to(dtype).contiguous(), Vs.to(dtype).contiguous()


def with_rows(scene, rows, drop_last=0):
    """The scene's Gaussians followed by those of every clamp_rows() dict in ``rows`` (less the last ``drop_last`` of
    each).  Adds groups (name -> rows of all the dicts) and culled (name -> list of rows)."""
    names = ("means", "quats", "scales", "opacities", "rgbs")
    out = dict(scene)
    parts = {k: [scene[k]] for k in names}
    groups = {name: [] for name in CLAMP_GROUPS}
    culled = {name: [] for name in CULL_ROWS[:len(CULL_ROWS) - drop_last]}
    start = scene["means"].shape[0]
    for r in rows:
        n = r["means"].shape[0] - drop_last
        for k in names:
            parts[k].append(r[k][:n].to(scene[k].dtype))
        for name in groups:
            groups[name].append(start + r["groups"][name])
        for name in culled:
            culled[name].append(start + r["culled"][name])
        start += n
    out.update({k: torch.cat(v).contiguous() for k, v in parts.items()})
    out.update(groups={k: torch.cat(v) for k, v in groups.items()} if rows else {}, culled=culled, N=start)
    return out


# ---- the inputs of the tests, shared by the CPU and the GPU files (float32, on the host) -------------------------------
F32 = torch.float32


@functools.lru_cache(maxsize=None)
def projection_case():
    """three_cameras on 96x64 (the last tile row is whole, x: 6 tiles): 2500 anisotropic splats spread over the control
    camera's image -- the widest of the three, so the others see a part of them -- and the clamp rows of wide_x and of
    wide_y."""
    W, H = 96, 64
    sc = camera_scene(2500, W, H, skewed_K(W, H, "control"), seed=7, sigma_px=1.5, aniso=True, dtype=F32)
    sc = with_rows(sc, [clamp_rows(skewed_K(W, H, which), W, H, seed=31 + i, dtype=F32)
                        for i, which in enumerate(CAMERAS[:2])])
    Ks, Vs = three_cameras(W, H, dtype=F32)
    sc.update(Ks=Ks, Vs=Vs, kw=dict(CLAMP_KW))
    return sc


STAGED_CASES = {  # render mode, SH degree (None: colours [N,3]), SH bands, antialiased, backgrounds, packed pipeline
    "sh2": dict(mode="RGB+ED", sh=2, bands=9, aa=False, bg=False, packed=False),
    "sh1-antialiased-bg": dict(mode="RGB+ED", sh=1, bands=4, aa=True, bg=True, packed=False),
    "ed": dict(mode="ED", sh=None, bands=0, aa=False, bg=False, packed=False),
    "rgb-packed": dict(mode="RGB", sh=None, bands=0, aa=False, bg=False, packed=True),
}


@functools.lru_cache(maxsize=None)
def staged_case(name):
    """(ins, Ks, kw, scene) of rasterization() on three_cameras, 100x70 (7 x 5 tiles, the last column 4 px and the last
    row 6 px wide): 2000 anisotropic splats of sigma ~ 2 px over the control camera's image and the clamp rows of wide_x
    and wide_y.  ins / Ks / kw as tests/staged_widths.py's oracle_e2e takes them."""
    case = STAGED_CASES[name]
    W, H = 100, 70
    sc = camera_scene(2000, W, H, skewed_K(W, H, "control"), seed=9, sigma_px=2.0, aniso=True, opacity=(0.1, 0.7), dtype=F32)
    sc = with_rows(sc, [clamp_rows(skewed_K(W, H, which), W, H, seed=41 + i, dtype=F32)
                        for i, which in enumerate(CAMERAS[:2])])
    n = sc["N"]
    gen = torch.Generator().manual_seed(31)
    colors = sc["rgbs"] if case["sh"] is None else 0.3 * torch.randn(n, case["bands"], 3, generator=gen)
    Ks, Vs = three_cameras(W, H, dtype=F32)
    ins = {k: sc[k] for k in ("means", "quats", "scales", "opacities")}
    ins.update(colors=colors.contiguous(), viewmats=Vs, backgrounds=torch.rand(3, 3, generator=gen) if case["bg"] else None)
    kw = dict(width=W, height=H, sh_degree=case["sh"], render_mode=case["mode"],
              rasterize_mode="antialiased" if case["aa"] else "classic", **CLAMP_KW)
    return ins, Ks, kw, sc


FUSED_CASES = {  # camera, render mode, splat size, and what RenderContext is built with
    "general-wide_x": dict(cam="wide_x", mode="RGB+ED", sigma=2.5, clamp=True, ctx={}),
    "general-wide_y": dict(cam="wide_y", mode="RGB+ED", sigma=2.5, clamp=True, ctx={}),
    "tiny-wide_x": dict(cam="wide_x", mode="ED", sigma=0.0, clamp=False, ctx={}),
    "antialiased-deterministic-wide_y": dict(cam="wide_y", mode="RGB+ED", sigma=1.5, clamp=False,
                                             ctx=dict(antialiased=True, deterministic=True)),
    "fp16-wide_x": dict(cam="wide_x", mode="RGB+ED", sigma=1.5, clamp=False, ctx=dict(staging="fp16")),
    "strip-wide_y": dict(cam="wide_y", mode="RGB+ED", sigma=1.5, clamp=False, ctx=dict(tile_rows=(1, 3))),
}


@functools.lru_cache(maxsize=None)
def fused_case(name):
    """One camera on 100x70: 2500 splats over THIS camera's image (anisotropic but for the tiny case: scales 0, every
    splat the 0.3 px^2 blur), SH coefficients of degree 1, a pose 1 degree and 3 cm off the identity; the general cases
    add this camera's clamp rows less the radius_clip one (the one-camera oracle has no radius_clip) with far_plane."""
    case = FUSED_CASES[name]
    W, H = 100, 70
    K = skewed_K(W, H, case["cam"])
    tiny = case["sigma"] == 0.0
    sc = camera_scene(2500, W, H, K, seed=13 if case["cam"] == "wide_x" else 14, sigma_px=case["sigma"], aniso=not tiny,
                      opacity=None if tiny else (0.1, 0.7), dtype=F32)
    rows = [clamp_rows(K, W, H, seed=51, dtype=F32)] if case["clamp"] else []
    sc = with_rows(sc, rows, drop_last=1)
    gen = torch.Generator().manual_seed(17)
    sc["sh"] = (0.3 * torch.randn(sc["N"], 4, 3, generator=gen)).contiguous()
    sc["V"] = torch.linalg.inv(small_pose(1.0, 0.03, seed=6)).float().contiguous()
    sc["K"] = K.float().contiguous()
    sc["planes"] = dict(near_plane=CLAMP_KW["near_plane"], far_plane=CLAMP_KW["far_plane"]) if case["clamp"] else {}
    return sc
