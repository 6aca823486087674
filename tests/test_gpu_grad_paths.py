"""Per-Gaussian gradients of every compositing path of RenderContext against float64 autograd of the oracle.

Each case forces one path -- the general atomic backward, the tiny-splat backward, the deterministic backward, long
lists split over workgroups, the forward that sorts its own bins, two-pass binning, tile-order placement, a tile-row
strip with pixel rows, and fp16-staged records crossed with several of these -- asserts that the path ran, and compares
render, alpha and every input gradient (means, quats, scales, opacities, colours / SH coefficients, viewmat) element by
element with the oracle on the same float32 inputs (fp16 records: with the oracle of tests/grad_paths.py that rounds what
a half record holds).  Flip-aware as tests/parity.py describes.

The scene is a "ladder" on a 200x136 image (the last tile column and row are 8 px wide): chosen tiles hold small
anisotropic splats whose lists have prescribed lengths around the kernels' batch, sort and segment sizes, around them
random background splats, and a few culled ones.  Outlier Gaussians are counted overall and within each targeted subset;
every case also shows that the comparator rejects the same gradients rolled by one row within each tile.
"""
import functools

import pytest
import torch

from tests import walk_ref as WR
from tests.grad_paths import compare_grads, failing_subsets, oracle_render, roll_within
from tests.parity import POSE_GRAD_TOL, agreeing_pixels, rel_inf, report
from tests.scenes import small_pose

pytestmark = pytest.mark.gpu

DEV = "cuda"
W, H, FX = 200, 136, 180.0
TW, TH = (W + 15) // 16, (H + 15) // 16  # 13 x 9 tiles
# (tx, ty) -> list length: around the compositing batches (64, 256) and the 1024-key sorts; edge tiles in column 12 / row 8
LADDER = {(0, 0): 1, (12, 0): 2, (2, 2): 63, (4, 2): 64, (6, 2): 65, (8, 2): 255, (10, 2): 256, (12, 2): 257,
          (2, 4): 1023, (6, 4): 1024, (12, 8): 1025}
# the "long" scene adds lists at LONG_MIN (2048: not yet long), past it, and at gsl_long_segment() (128) multiples +- 1
LONG = {(4, 6): 2048, (8, 6): 2049, (10, 4): 2303, (0, 8): 2561}
SUBSETS = {"<=65": (1, 65), "255-257": (255, 257), "1023-1025": (1023, 1025), "long": (2048, 1 << 30)}
N_BACKGROUND = 1500
MAX_FLIPPED = 3e-3  # pixels sitting on a compositing threshold (test_fused_full_gradients' bound)
STRIP = dict(tile_rows=(2, 9), pixel_rows=(35, 133))
NAMES = ("means", "quats", "scales", "opacities", "colors")

M3 = ("RGB+ED", "ED", "RGB")
M5 = M3 + ("D", "RGB+D")
PATHS = {  # path: (scene, staging, render modes)
    "general": ("ladder", "fp32", M5),
    "tiny": ("tiny", "fp32", M3),
    "deterministic": ("ladder", "fp32", M3),
    "long": ("long", "fp32", M3),
    "sort-in-forward": ("ladder", "fp32", M3),
    "two-pass": ("ladder", "fp32", M3),
    "placement": ("ladder", "fp32", M3),
    "strip": ("ladder", "fp32", M3),
    "fp16-general": ("ladder", "fp16", M5),
    "fp16-deterministic": ("ladder", "fp16", M3),
    "fp16-long": ("long", "fp16", M3),
    "fp16-strip": ("ladder", "fp16", M3),
    "fp16-placement": ("ladder", "fp16", M3),
    "fp16-tiny": ("tiny", "fp16", ("RGB+ED",)),  # fp16 records exclude the tiny backward: the general one runs
}


def _back_project(u, v, z, c2w, fx, cx, cy):
    """World points that the camera inv(c2w) sees at pixel (u, v) and depth z."""
    cam = torch.stack([(u - cx) / fx * z, (v - cy) / fx * z, z], -1)
    return cam @ c2w[:3, :3].T + c2w[:3, 3]


def pose_key(c2w):
    """A camera-to-world matrix as a hashable key of the scene and oracle caches."""
    return tuple(float(x) for x in torch.as_tensor(c2w, dtype=torch.float64).reshape(-1).tolist())


@functools.lru_cache(maxsize=None)
def _ladder_scene(variant, c2w=None):
    """float32 inputs of the ladder scene ("ladder"; "tiny": every splat below 0.1 px; "long": with the long tiles), in a
    shuffled Gaussian order, and the index sets the checks use.  The scene is built on screen and back-projected through
    the camera ``c2w`` (a pose_key(); default: next to the identity), so another pose moves the world, not the image."""
    g = torch.Generator().manual_seed({"ladder": 1, "tiny": 2, "long": 3}[variant])
    f64 = torch.float64
    cx, cy = W / 2.0, H / 2.0
    tiny = variant == "tiny"
    tiles = {**LADDER, **(LONG if variant == "long" else {})}
    U, V, Z, S, O, tile_of = [], [], [], [], [], []
    for (tx, ty), n in tiles.items():
        # centres >= 5 px inside the tile's left and top border and <= 11 px from it: radius <= 4 keeps each splat in its
        # tile's list only (ragged tiles: inside the image)
        x0, y0 = 16.0 * tx, 16.0 * ty
        xs, ys = min(x0 + 11.0, W - 0.5) - x0 - 5.0, min(y0 + 11.0, H - 0.5) - y0 - 5.0
        U.append(x0 + 5.0 + xs * torch.rand(n, generator=g, dtype=f64))
        V.append(y0 + 5.0 + ys * torch.rand(n, generator=g, dtype=f64))
        Z.append(1.5 + 2.5 * torch.rand(n, generator=g, dtype=f64))
        S.append((0.02 + 0.06 * torch.rand(n, generator=g, dtype=f64)) if tiny else
                 (0.3 + 0.3 * torch.rand(n, generator=g, dtype=f64)))
        lo, hi = (0.01, 0.02) if n >= 2048 else (0.04, min(0.95, max(0.08, 40.0 / n)))  # long walks: low opacity
        O.append(lo + (hi - lo) * torch.rand(n, generator=g, dtype=f64))
        tile_of += [(tx, ty)] * n
    # background: random splats whose (generous) tile rectangle stays off every ladder tile of any variant
    m = 8 * N_BACKGROUND
    u, v = W * torch.rand(m, generator=g, dtype=f64), H * torch.rand(m, generator=g, dtype=f64)
    s = (0.02 + 0.06 * torch.rand(m, generator=g, dtype=f64)) if tiny else (0.5 + 2.0 * torch.rand(m, generator=g, dtype=f64))
    R = 3.0 * torch.sqrt((1.8 * s) ** 2 + 0.3) + 2.0
    keep = torch.ones(m, dtype=torch.bool)
    for tx, ty in list(LADDER) + list(LONG):
        keep &= ~((torch.floor((u + R) / 16) >= tx) & (torch.floor((u - R) / 16) <= tx)
                  & (torch.floor((v + R) / 16) >= ty) & (torch.floor((v - R) / 16) <= ty))
    idx = keep.nonzero()[:, 0][:N_BACKGROUND]
    assert idx.numel() == N_BACKGROUND
    U.append(u[idx])
    V.append(v[idx])
    Z.append(1.0 + 4.0 * torch.rand(N_BACKGROUND, generator=g, dtype=f64))
    S.append(s[idx])
    O.append(0.05 + 0.9 * torch.rand(N_BACKGROUND, generator=g, dtype=f64))
    tile_of += [(int(a) // 16, int(b) // 16) for a, b in zip(u[idx].tolist(), v[idx].tolist())]
    n_vis = sum(t.numel() for t in U)
    # culled: behind the camera, in front of the near plane (0.01), off screen
    U.append(torch.tensor([50.0, 120.0, 60.0, 150.0, -80.0, 290.0], dtype=f64))
    V.append(torch.tensor([40.0, 90.0, 20.0, 100.0, 60.0, 40.0], dtype=f64))
    Z.append(torch.tensor([-2.0, -0.5, 0.005, 0.002, 3.0, 2.0], dtype=f64))
    S.append(torch.full((6,), 0.05 if tiny else 1.0, dtype=f64))
    O.append(torch.full((6,), 0.8, dtype=f64))
    U, V, Z, S, O = (torch.cat(t) for t in (U, V, Z, S, O))
    N = U.numel()
    c2w = small_pose(0.4, 0.01, seed=5) if c2w is None else torch.tensor(c2w, dtype=f64).reshape(4, 4)
    means = _back_project(U, V, Z, c2w, FX, cx, cy)
    quats = torch.randn(N, 4, generator=g, dtype=f64)
    scales = (S * Z.abs() / FX)[:, None] * (0.6 + 0.8 * torch.rand(N, 3, generator=g, dtype=f64))
    sh = 0.3 * torch.randn(N, 4, 3, generator=g, dtype=f64)
    rgb = torch.rand(N, 3, generator=g, dtype=f64)
    K = torch.tensor([[FX, 0, cx], [0, FX, cy], [0, 0, 1]], dtype=f64)
    # shuffled order: placement has work to do, and a tile's Gaussians are not one contiguous block
    perm = torch.randperm(N, generator=g)
    pos = torch.empty_like(perm)
    pos[perm] = torch.arange(N)  # new index of old Gaussian i
    f32 = lambda t: t[perm].float().contiguous()  # noqa: E731
    groups, subsets = [], {"all": pos[:n_vis]}
    start = 0
    for (tx, ty), n in tiles.items():
        groups.append(pos[start:start + n])
        start += n
    groups.append(pos[start:n_vis])  # the background
    for name, (lo, hi) in SUBSETS.items():
        sel = [grp for grp, n in zip(groups, tiles.values()) if lo <= n <= hi]
        if sel:
            subsets[name] = torch.cat(sel)
    edge = torch.tensor([tx == TW - 1 or ty == TH - 1 for tx, ty in tile_of])
    subsets["edge"] = pos[:n_vis][edge]
    return dict(N=N, means=f32(means), quats=f32(quats), scales=f32(scales), opacities=f32(O), sh=f32(sh), rgb=f32(rgb),
                V=torch.linalg.inv(c2w).float().contiguous(), K=K.float(), groups=groups, subsets=subsets,
                culled=pos[n_vis:], lengths=tiles)


_ORACLE = {}
_EXPLAINED = set()


def _oracle(variant, mode, half, c2w=None):
    """The oracle's forward on the scene (kept for the next case with the same scene, pose, mode and rounding)."""
    key = (variant, mode, half, c2w)
    if key not in _ORACLE:
        _ORACLE.clear()
        sc = _ladder_scene(variant, c2w)
        sh = 1 if mode in ("RGB+ED", "RGB+D") else None
        leaves = {k: sc[k].double().requires_grad_() for k in ("means", "quats", "scales", "opacities")}
        if mode.startswith("RGB"):
            leaves["colors"] = (sc["sh"] if sh is not None else sc["rgb"]).double().requires_grad_()
        leaves["viewmat"] = sc["V"].double().requires_grad_()
        r, a = oracle_render(leaves["means"], leaves["quats"], leaves["scales"], leaves["opacities"],
                             leaves.get("colors"), leaves["viewmat"], sc["K"].double(), W, H, mode, sh_degree=sh,
                             half=half)
        _ORACLE[key] = (leaves, r, a)
    return _ORACLE[key]


def _oracle_grads(entry, v, va):
    leaves, r, a = entry
    names = list(leaves)
    gs = torch.autograd.grad([r, a], [leaves[k] for k in names], grad_outputs=[v, va], retain_graph=True,
                             allow_unused=True)
    return {k: (t if t is not None else torch.zeros_like(leaves[k])) for k, t in zip(names, gs)}


def _upstream(kind, D, ok):
    """random: every channel and alpha; tracker: the depth channel only; mixed: depth everywhere, RGB in a few tiles
    (whole tiles, one quadrant, one pixel of the ragged corner) -- the depth-only backward hands those quadrants over."""
    gen = torch.Generator().manual_seed(17)
    v = torch.randn(H, W, D, generator=gen, dtype=torch.float64)
    va = torch.randn(H, W, 1, generator=gen, dtype=torch.float64)
    if kind != "random":
        v[..., :3] = 0.0
        if kind == "tracker":
            va.zero_()
        else:
            for tx, ty in ((2, 2), (8, 2)):
                v[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16, :3] = torch.randn(16, 16, 3, generator=gen, dtype=torch.float64)
            v[64:72, 104:112, :3] = torch.randn(8, 8, 3, generator=gen, dtype=torch.float64)  # one quadrant of (6, 4)
            v[133, 198, :3] = torch.tensor([0.7, -0.4, 0.2], dtype=torch.float64)
    return v * ok[..., None], va * ok[..., None]


def _cases():
    out = []
    for path, (variant, staging, modes) in PATHS.items():
        for mode in modes:
            for up in (("random", "tracker", "mixed") if mode == "RGB+ED" else ("random",)):
                out.append((variant, staging, mode, path, up))
    out.sort(key=lambda c: c[:3])  # consecutive cases share one oracle forward
    return [pytest.param(c[3], c[2], c[4], id=f"{c[3]}-{c[2]}-{c[4]}") for c in out]


def _check_gaussian_grads(tag, g, want, sc):
    """Element bound per Gaussian and subset, zero rows of the culled, and the comparator's teeth (rolled rows)."""
    names = [nm for nm in NAMES if nm in want]
    got = {nm: g[nm] for nm in names}
    ref = {nm: want[nm] for nm in names}
    worst, counts, _ = compare_grads(got, ref, sc["subsets"])
    for nm in names:
        rows = got[nm].detach().cpu()[sc["culled"]]
        assert float(rows.abs().max()) == 0.0, (tag, "culled Gaussian with a gradient", nm)
    _, rolled, _ = compare_grads(roll_within(got, sc["groups"]), ref, sc["subsets"])
    return worst, counts, rolled


@pytest.mark.parametrize("path,mode,upstream", _cases())
def test_per_gaussian_gradients_of_every_compositing_path(path, mode, upstream, monkeypatch):
    run_path_case(path, mode, upstream, monkeypatch)


def run_path_case(path, mode, upstream, monkeypatch, c2w=None, label="grad paths", pose_tol=None):
    """One case of the matrix: force the path, assert that it ran, compare with the oracle.  ``c2w`` (a pose_key())
    builds the scene at another camera (tests/test_gpu_far_pose.py); ``pose_tol(tag, sc, mode, half, oracle, v, va)``
    returns the bound of the view-matrix gradient for a case there that misses POSE_GRAD_TOL."""
    from gsplatloc_amd.context import RenderContext
    variant, staging, _ = PATHS[path]
    base = path.replace("fp16-", "")
    sc = _ladder_scene(variant, c2w)
    monkeypatch.setenv("GSLOC_BWD", "tiny" if base == "tiny" else "general")
    if base == "sort-in-forward":
        monkeypatch.setenv("GSLOC_SORT_IN_FORWARD", "force")
    if base == "two-pass":
        monkeypatch.setenv("GSLOC_BINNING", "two-pass")
    rgb = mode.startswith("RGB")
    sh = 1 if mode in ("RGB+ED", "RGB+D") else None
    kw = dict(STRIP) if base == "strip" else {}
    rc = RenderContext(sc["N"], W, H, mode, sh_degree=sh, K_sh=4, device=DEV, full_grads=True, staging=staging,
                       deterministic=base == "deterministic", reorder=base == "placement",
                       sort_in_forward=base == "sort-in-forward", **kw)
    colors = (sc["sh"] if sh is not None else sc["rgb"]) if rgb else None
    ins = [sc[k].to(DEV) for k in ("means", "quats", "scales", "opacities")] + [
        colors.to(DEV) if rgb else None, sc["V"].to(DEV), sc["K"].to(DEV)]
    rc.calibrate(*ins)
    sizes = (rc.offs[1:] - rc.offs[:-1]).cpu()
    if base != "strip":  # the ladder is what it says
        assert {t: int(sizes[t[1] * TW + t[0]]) for t in sc["lengths"]} == sc["lengths"]
    # the path ran
    assert rc.tiny == (path == "tiny"), path
    assert (rc.Qh is not None) == (staging == "fp16")
    assert (rc.vrow is not None) == (base == "deterministic")
    assert (rc.long_min > 0) == (base == "long")
    assert rc.sorts_in_forward() == (base == "sort-in-forward")
    assert (rc.bins is None) == (base == "two-pass")
    assert (rc.order_ids is not None) == (base == "placement")
    render, alphas = rc.forward(*ins)
    if base == "long":
        assert int(rc.long_ws[:16].view(torch.int32)[0]) > 0, "no long-list segment was composited"
    rc.check_capacity()
    leaves, r_o, a_o = _oracle(variant, mode, staging == "fp16", c2w)
    y0, y1 = rc.row0, rc.row1
    rg, ag = render.cpu().double(), alphas.cpu().double()
    ok = agreeing_pixels(rg, ag, r_o.detach(), a_o.detach())
    ok[:y0] = False
    ok[y1:] = False
    flipped = 1.0 - ok[y0:y1].double().mean().item()
    tag = f"{label} {path} {mode} {upstream}"
    assert flipped <= MAX_FLIPPED, f"{tag}: {flipped:.2e} of the pixels differ from the oracle"
    if (label, path, mode, c2w) not in _EXPLAINED:  # once per (scene, path, mode), not once per upstream kind
        # every pixel rejected above, and every pixel that differs from the walk of the context's own records, sits on a
        # compositing threshold and is what the walk gives with that decision taken the other way (tests/walk_ref.py)
        suspects = ~ok
        suspects[:y0] = False
        suspects[y1:] = False
        WR.assert_flips_explained(f"{label} {path} {mode}", rc, render, alphas, suspects, oracle=(r_o, a_o))
        _EXPLAINED.add((label, path, mode, c2w))
    if staging == "fp16" and base == "general" and upstream == "random":
        # the rounding is what is modelled: against the unrounded oracle the fp16 render misses 1e-4 somewhere
        with torch.no_grad():
            r_p, a_p = oracle_render(*[leaves[k] for k in ("means", "quats", "scales", "opacities")],
                                     leaves.get("colors"), leaves["viewmat"], sc["K"].double(), W, H, mode, sh_degree=sh)
        assert not bool(agreeing_pixels(rg, ag, r_p, a_p).all()), f"{tag}: fp16 render meets 1e-4 without the rounding"
    v, va = _upstream(upstream, rc.D, ok)
    want = _oracle_grads((leaves, r_o, a_o), v, va)
    floor_tol = []

    def tol_for(err):  # POSE_GRAD_TOL; a case that misses it may have its own float32 floor measured (once)
        if err < POSE_GRAD_TOL or pose_tol is None:
            return POSE_GRAD_TOL
        if not floor_tol:
            floor_tol.append(pose_tol(tag, sc, mode, staging == "fp16", (leaves, r_o, a_o), v, va))
        return floor_tol[0]

    vg, vag = v.float().to(DEV).contiguous(), va.float().to(DEV).contiguous()
    for it in range(2):  # twice: accumulators, slabs, rows and counters must come back clean
        if it:
            rc.forward(*ins)
        g = rc.backward(vg, vag, full=upstream != "tracker" or it == 1)
        if upstream == "tracker" and it == 0:  # the tracker's call: pose gradient only
            err0 = rel_inf(g["viewmat"][:3], want["viewmat"][:3])
            assert err0 < tol_for(err0), (tag, "full=False", err0)
    g = {k: (t.clone() if t is not None else None) for k, t in rc.grads_in_input_order(g).items()}
    err_v = rel_inf(g["viewmat"][:3], want["viewmat"][:3])
    worst, counts, rolled = _check_gaussian_grads(tag, g, want, sc)
    report(tag, flipped, v_viewmat=err_v, **{"v_" + k: x for k, x in worst.items()},
           **{"outliers " + k: float(c[0]) for k, c in counts.items()},
           **{"rolled outliers " + k: float(c[0]) for k, c in rolled.items()})
    assert err_v < tol_for(err_v), (tag, err_v)
    assert not failing_subsets(counts), (tag, "outlier Gaussians (count, size, allowed)", counts, worst)
    assert set(failing_subsets(rolled)) == set(counts), (tag, "rolled rows not rejected in every subset", rolled)


def _far_scene(depth):
    """64x48: 400 splats at depth 1..4 and 12 large ones at `depth` (beyond the half range at 1e5), partly uncovered."""
    g = torch.Generator().manual_seed(int(depth) % 1000 + 5)
    f64 = torch.float64
    Wf, Hf, fx = 64, 48, 50.0
    n_near, n_far = 400, 12
    u = torch.cat([Wf * torch.rand(n_near, generator=g, dtype=f64), 4.0 + (Wf - 8.0) * torch.rand(n_far, generator=g, dtype=f64)])
    v = torch.cat([Hf * torch.rand(n_near, generator=g, dtype=f64), 4.0 + (Hf - 8.0) * torch.rand(n_far, generator=g, dtype=f64)])
    z = torch.cat([1.0 + 3.0 * torch.rand(n_near, generator=g, dtype=f64), depth * (1.0 + 0.1 * torch.rand(n_far, generator=g, dtype=f64))])
    s = torch.cat([0.5 + 1.0 * torch.rand(n_near, generator=g, dtype=f64), 3.0 + 2.0 * torch.rand(n_far, generator=g, dtype=f64)])
    op = torch.cat([0.1 + 0.5 * torch.rand(n_near, generator=g, dtype=f64), 0.6 + 0.35 * torch.rand(n_far, generator=g, dtype=f64)])
    N = n_near + n_far
    c2w = small_pose(0.3, 0.01, seed=9)
    means = _back_project(u, v, z, c2w, fx, Wf / 2.0, Hf / 2.0)
    scales = (s * z / fx)[:, None] * (0.7 + 0.6 * torch.rand(N, 3, generator=g, dtype=f64))
    K = torch.tensor([[fx, 0, Wf / 2.0], [0, fx, Hf / 2.0], [0, 0, 1]], dtype=f64)
    f32 = lambda t: t.float().contiguous()  # noqa: E731  (linalg.inv returns a column-major matrix)
    return dict(W=Wf, H=Hf, means=f32(means), quats=f32(torch.randn(N, 4, generator=g)), scales=f32(scales),
                opacities=f32(op), sh=f32(0.3 * torch.randn(N, 4, 3, generator=g)), V=f32(torch.linalg.inv(c2w)),
                K=f32(K), far=torch.arange(n_near, N))


@pytest.mark.parametrize("depth", [3e4, 1e5])
@pytest.mark.parametrize("mode", ["ED", "RGB+ED"])
def test_fp16_records_keep_depths_beyond_the_half_range(mode, depth, monkeypatch):
    """Visible Gaussians at camera-space depth 3e4 and 1e5 under staging="fp16": the depth channel is finite and matches
    the oracle, and so do the gradients -- the half record carries the depth feature as float32 (1e5 used to become
    +inf in the half, 3e4 kept 11 significant bits)."""
    from gsplatloc_amd.context import RenderContext
    monkeypatch.setenv("GSLOC_BWD", "general")
    sc = _far_scene(depth)
    Wf, Hf, N = sc["W"], sc["H"], sc["means"].shape[0]
    sh = 1 if mode == "RGB+ED" else None
    rc = RenderContext(N, Wf, Hf, mode, sh_degree=sh, K_sh=4, device=DEV, full_grads=True, staging="fp16")
    ins = [sc[k].to(DEV) for k in ("means", "quats", "scales", "opacities")] + [
        sc["sh"].to(DEV) if sh else None, sc["V"].to(DEV), sc["K"].to(DEV)]
    rc.calibrate(*ins)
    render, alphas = rc.forward(*ins)
    rc.check_capacity()
    assert bool(torch.isfinite(render).all()) and bool(torch.isfinite(alphas).all()), "non-finite render"
    leaves = {k: sc[k].double().requires_grad_() for k in ("means", "quats", "scales", "opacities")}
    if sh:
        leaves["colors"] = sc["sh"].double().requires_grad_()
    leaves["viewmat"] = sc["V"].double().requires_grad_()
    r_o, a_o = oracle_render(leaves["means"], leaves["quats"], leaves["scales"], leaves["opacities"],
                             leaves.get("colors"), leaves["viewmat"], sc["K"].double(), Wf, Hf, mode, sh_degree=sh,
                             half=True)
    assert float(r_o[..., -1].max()) > 0.5 * depth  # the far splats are seen
    rg, ag = render.cpu().double(), alphas.cpu().double()
    ok = agreeing_pixels(rg, ag, r_o.detach(), a_o.detach())
    flipped = 1.0 - ok.double().mean().item()
    tag = f"fp16 far depth {depth:g} {mode}"
    assert flipped <= MAX_FLIPPED, f"{tag}: {flipped:.2e} of the pixels differ from the oracle"
    gen = torch.Generator().manual_seed(3)
    v = torch.randn(Hf, Wf, rc.D, generator=gen, dtype=torch.float64) * ok[..., None]
    va = torch.randn(Hf, Wf, 1, generator=gen, dtype=torch.float64) * ok[..., None]
    want = _oracle_grads((leaves, r_o, a_o), v, va)
    g = rc.backward(v.float().to(DEV).contiguous(), va.float().to(DEV).contiguous())
    names = [nm for nm in NAMES if nm in want]
    subsets = {"all": torch.arange(N), "far": sc["far"]}
    worst, counts, _ = compare_grads({nm: g[nm] for nm in names}, {nm: want[nm] for nm in names}, subsets)
    err_v = rel_inf(g["viewmat"][:3], want["viewmat"][:3])
    report(tag, flipped, v_viewmat=err_v, **{"v_" + k: x for k, x in worst.items()},
           **{"outliers " + k: float(c[0]) for k, c in counts.items()})
    assert err_v < POSE_GRAD_TOL, (tag, err_v)
    assert not failing_subsets(counts), (tag, counts, worst)


def test_fp16_staging_refuses_an_eps2d_whose_conic_leaves_the_half_range():
    """A degenerate splat's conic reaches 1/eps2d; as a half it must stay below 65504."""
    from gsplatloc_amd.context import FP16_EPS2D_MIN, RenderContext
    with pytest.raises(ValueError, match="eps2d"):
        RenderContext(16, 32, 32, "RGB+ED", device=DEV, staging="fp16", eps2d=1e-5)
    assert 1.0 / FP16_EPS2D_MIN < 65504.0
    RenderContext(16, 32, 32, "RGB+ED", device=DEV, staging="fp16", eps2d=FP16_EPS2D_MIN)
    RenderContext(16, 32, 32, "RGB+ED", device=DEV, staging="fp32", eps2d=1e-5)  # float32 records have the range
