"""The compositing forward at the shapes where its per-batch work can go wrong (k_praster_fwd, praster_walk and
compact_quadrants in gsplatloc_amd/csrc/raster_px.hip): tile lists that end just before, on and just after a batch (256
records) or a chunk (64 candidates) boundary, per-quadrant candidate counts of zero, full quadrant lists whose bases are
exactly 0 / 64 / 128 / 192, and a random mix -- each at opacity 0.05 (every batch is walked; at most the pile of the
"centre" scene saturates, late) and at opacity 1 (pixels stop early), with the separate sort launch and with the forward
that sorts its own bins.

Checker: the float64 C oracle (oracle/c_oracle.py).  Images at the tolerance of tests/parity.py with at most 0.1 % of the
pixels outside (the seeds are such that the oracle's own float32 build stays inside that against its float64 build:
test_the_seeds_keep_the_float32_oracle_inside_the_cap, no GPU needed), n_isects equal, pose gradient and per-Gaussian
gradients on the agreeing pixels (the general backward walks the hit lists the forward wrote), the hit lists'
invariants, and bit-identical results whatever LDS held before the launch.

Gradient bounds: per Gaussian the element bound of tests/grad_paths.py; the pose gradient within tests/parity.py's
pose_grad_bound(float32 floor, kind) -- the cap of the kind of splats ("subpixel" for the sigma 0.6 px and 0.1 px scenes,
"sigma1" for "centre" and "mix") or 1.25 x the floor measured in the same test, the oracle's own float32 build against
its float64 build on the same upstream gradient; the floor itself is bounded by FLOOR32_MAX.  parity.py's flat
POSE_GRAD_TOL (1e-4 of the largest entry) does not apply to these scenes: they are a handful of splats on a few dozen
pixels, nothing averages out, and the float32 ORACLE sits at 1.5e-4 from the float64 one on "list1" at opacity 0.05 and
on "mix" at opacity 1, and at 1.0e-4 on "quadrant0" at opacity 1 (2e-5 typically elsewhere).  Nor is 1.25 x one draw of
that floor alone a bound (parity.py: "a bound derived from one draw of the floor is itself a coin flip"): measured on
MI355X, "quadrant0" at opacity 1 gives 1.96e-4 against a floor of 1.04e-4 -- with the general and with the tiny
backward, and with the library as it was before the per-batch compaction was rewritten, alike -- and everything else
stays below 1.5e-4 (up to 2.5 x its own floor, at 3e-5).  Every figure is printed before it is asserted.

"quadrant 0": the 0.3 px^2 blur alone gives r_cull = 1.24 px at opacity 0.05 and 1.87 px at opacity 1, so r_cull < 1 px
cannot be had at these opacities; the centres keep more than r_cull + 3.5 px from the centres of the other three
quadrants instead, which is what makes their counts zero (asserted: their hit lists are empty and their pixels blank).
"""
import functools

import numpy as np
import pytest
import torch

from tests.grad_paths import compare_grads, failing_subsets
from tests.parity import FLOOR32_MAX, agreeing_pixels, pose_grad_bound, rel_inf
from tests.scenes import random_scene, sh_from_rgb

LIST_SIZES = (1, 63, 64, 65, 255, 256, 257, 300, 513)
SCENES = tuple(f"list{n}" for n in LIST_SIZES) + ("quadrant0", "centre", "mix")
TINY_SCENES = ("quadrant0", "blur257")  # every r_cull < 2 px: what the tiny-splat backward takes
OPACITIES = (0.05, 1.0)
MAX_OUTSIDE = 1e-3  # of the pixels
FX = 24.0


def _from_pixels(u, v, z, sigma_px, W, H, seed):
    """Isotropic Gaussians with projected centres (u, v) px, depths z and sigma_px px, seen from the identity pose."""
    g = torch.Generator().manual_seed(seed + 1000)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    N = u.numel()
    means = torch.stack([(u - cx) / FX * z, (v - cy) / FX * z, z], -1)
    scales = (sigma_px * z / FX)[:, None].repeat(1, 3)
    quats = torch.tensor([1.0, 0, 0, 0], dtype=torch.float64).repeat(N, 1)
    K = torch.tensor([[FX, 0, cx], [0, FX, cy], [0, 0, 1]], dtype=torch.float64)
    return dict(means=means, quats=quats, scales=scales, rgbs=torch.rand(N, 3, generator=g, dtype=torch.float64), K=K)


@functools.lru_cache(maxsize=None)
def _scene(name, opacity):
    """float32 inputs (what both sides get), the image size and the tile whose list the scene is about."""
    g = torch.Generator().manual_seed(SEEDS[name])
    rnd = lambda n: torch.rand(n, generator=g, dtype=torch.float64)  # noqa: E731
    tile = None
    if name.startswith("list"):
        # n splats of sigma 0.6 px (tile radius 3 px) whose boxes stay inside tile (1, 1) of a 32x32 image
        n, (W, H) = int(name[4:]), (32, 32)
        sc = _from_pixels(19.5 + 9.0 * rnd(n), 19.5 + 9.0 * rnd(n), 1.0 + 4.0 * rnd(n), torch.full((n,), 0.6, dtype=torch.float64),
                          W, H, SEEDS[name])
        tile = (1, 1, n)
    elif name == "blur257":
        # a batch and one entry of sigma 0.1 px splats (the 0.3 px^2 blur: tile radius 2 px) all over tile (1, 1)
        n, (W, H) = 257, (32, 32)
        sc = _from_pixels(18.5 + 11.0 * rnd(n), 18.5 + 11.0 * rnd(n), 1.0 + 4.0 * rnd(n), torch.full((n,), 0.1, dtype=torch.float64),
                          W, H, SEEDS[name])
        tile = (1, 1, n)
    elif name == "quadrant0":
        n, (W, H) = 200, (16, 16)
        sc = _from_pixels(2.1 + 4.3 * rnd(n), 2.1 + 4.3 * rnd(n), 1.0 + 4.0 * rnd(n), torch.full((n,), 0.1, dtype=torch.float64),
                          W, H, SEEDS[name])
        tile = (0, 0, n)
    elif name == "centre":
        # one full batch (every wave's 64 records are candidates of all four quadrants) and a partial one
        n, (W, H) = 320, (16, 16)
        sc = _from_pixels(torch.full((n,), 8.0, dtype=torch.float64), torch.full((n,), 8.0, dtype=torch.float64),
                          1.0 + 4.0 * rnd(n), torch.full((n,), 2.0, dtype=torch.float64), W, H, SEEDS[name])
        tile = (0, 0, n)
    else:
        n, (W, H) = 1500, (48, 32)
        sc = random_scene(n, W, H, seed=SEEDS[name], sigma_px=1.2, fx=FX, aniso=True)
    sc = {k: (t.float() if torch.is_tensor(t) else t) for k, t in sc.items()}
    sc["opacities"] = torch.full((n,), opacity, dtype=torch.float32)
    sc["sh"] = sh_from_rgb(sc["rgbs"])
    sc["V"] = torch.eye(4, dtype=torch.float32)
    sc.update(N=n, W=W, H=H, tile=tile)
    return sc


# seeds for which the oracle's float32 build stays inside MAX_OUTSIDE against its float64 build at both opacities
SEEDS = {name: 11 + i for i, name in enumerate(SCENES + TINY_SCENES[1:])}


def _oracle_inputs(sc):
    return [sc[k] for k in ("means", "quats", "scales", "opacities", "sh")] + [sc["V"], sc["K"]]


@functools.lru_cache(maxsize=None)
def _oracle_forward(name, opacity, precision="f64"):
    from oracle import c_oracle as C
    sc = _scene(name, opacity)
    return C.rasterization(*_oracle_inputs(sc), sc["W"], sc["H"], sh_degree=1, render_mode="RGB+ED", precision=precision)


_ORACLE_BWD = {}


def _oracle_backward(name, opacity, kind, v, va):
    """The float64 oracle's gradients and the float32 floor of the pose gradient (the oracle's float32 build against
    them).  Cached per upstream gradient: the two contexts of a scene agree on the pixels and share it."""
    from oracle import c_oracle as C
    key = (name, opacity, kind, v.numpy().tobytes(), va.numpy().tobytes())
    if key not in _ORACLE_BWD:
        sc = _scene(name, opacity)
        ref, ref32 = (C.rasterization(*_oracle_inputs(sc), sc["W"], sc["H"], sh_degree=1, render_mode="RGB+ED",
                                      v_render=v, v_alphas=va[..., 0], precision=p) for p in ("f64", "f32"))
        _ORACLE_BWD[key] = (ref, rel_inf(ref32["v_viewmat"][:3], ref["v_viewmat"][:3]))
    return _ORACLE_BWD[key]


def _pose_bound(name, floor32):
    return pose_grad_bound(floor32, "sigma1" if name in ("centre", "mix") else "subpixel")


def _outside(a, b):
    ok = agreeing_pixels(torch.from_numpy(a["render"]), torch.from_numpy(a["alphas"])[..., None],
                         torch.from_numpy(b["render"]), torch.from_numpy(b["alphas"])[..., None])
    return 1.0 - ok.double().mean().item()


@pytest.mark.parametrize("opacity", OPACITIES)
@pytest.mark.parametrize("name", SCENES + TINY_SCENES[1:])
def test_the_seeds_keep_the_float32_oracle_inside_the_cap(name, opacity):
    f64, f32 = _oracle_forward(name, opacity), _oracle_forward(name, opacity, "f32")
    sc = _scene(name, opacity)
    assert f64["n_isects"] == f32["n_isects"]
    if sc["tile"] is not None:  # the scene is what it says: one tile list of n entries
        assert f64["n_isects"] == sc["tile"][2]
    assert _outside(f32, f64) <= MAX_OUTSIDE, (name, opacity, _outside(f32, f64))


def _upstream(kind, H, W, ok):
    gen = torch.Generator().manual_seed(17)
    v = torch.randn(H, W, 4, generator=gen, dtype=torch.float64)
    va = torch.randn(H, W, 1, generator=gen, dtype=torch.float64)
    if kind == "depth":  # the tracker's loss: depth channel only (the depth-only instance of the backward)
        v[..., :3] = 0.0
        va.zero_()
    return v * ok[..., None], va * ok[..., None]


def _check_hit_lists(rc, sc):
    """Per tile and quadrant: list indices strictly ascending and inside the tile's list, a non-zero group nibble in
    every word, no more hits than list entries."""
    offs = rc.offs.cpu().tolist()
    counts = rc.hit_counts.cpu().tolist()
    hits = rc.hits.cpu().numpy().view(np.uint32)
    total = 0
    for t in range(rc.n_tiles):
        rs, re = offs[t], offs[t + 1]
        for q in range(4):
            c = counts[4 * t + q]
            assert 0 <= c <= re - rs, (t, q, c, re - rs)
            w = hits[4 * rs + q * (re - rs): 4 * rs + q * (re - rs) + c]
            idx = (w & 0x0FFFFFFF).astype(np.int64)
            assert ((w >> 28) != 0).all(), (t, q, "a hit word without a pixel group")
            assert (np.diff(idx) > 0).all(), (t, q, "list indices not strictly ascending")
            if c:
                assert rs <= idx[0] and idx[-1] < re, (t, q, int(idx[0]), int(idx[-1]), rs, re)
            total += c
    return total


@pytest.mark.gpu
@pytest.mark.parametrize("sort_in_forward", [False, True], ids=["sort-launch", "sort-in-forward"])
@pytest.mark.parametrize("opacity", OPACITIES)
@pytest.mark.parametrize("name", SCENES)
def test_forward_batches_against_the_oracle(name, opacity, sort_in_forward, monkeypatch):
    from gsplatloc_amd._lib import check, current_stream, load_library
    from gsplatloc_amd.context import RenderContext

    assert torch.cuda.is_available()
    dev = torch.device("cuda")
    monkeypatch.setenv("GSLOC_BWD", "general")  # the backward that walks the forward's hit lists
    sc = _scene(name, opacity)
    N, W, H = sc["N"], sc["W"], sc["H"]
    tag = f"{name} opacity {opacity} {'sort-in-forward' if sort_in_forward else 'sort-launch'}"
    want = _oracle_forward(name, opacity)
    rc = RenderContext(N, W, H, "RGB+ED", sh_degree=1, K_sh=4, device=dev, full_grads=True, sort_in_forward=sort_in_forward)
    ins = [t.to(dev).contiguous() for t in _oracle_inputs(sc)]
    n_is = rc.calibrate(*ins)
    assert n_is == want["n_isects"], (tag, n_is, want["n_isects"])
    assert rc.sorts_in_forward() == sort_in_forward and not rc.tiny and rc.long_min == 0 and rc.Qh is None
    render, alphas = rc.forward(*ins)
    torch.cuda.synchronize()
    assert rc.check_capacity() == n_is
    if sc["tile"] is not None:
        tx, ty, n = sc["tile"]
        sizes = (rc.offs[1:] - rc.offs[:-1]).cpu().tolist()
        assert sizes[ty * rc.tw + tx] == n and sum(sizes) == n, (tag, sizes)
    first = (render.clone(), alphas.clone(), rc.hits.clone(), rc.hit_counts.clone())

    # images
    r_o, a_o = torch.from_numpy(want["render"]), torch.from_numpy(want["alphas"])[..., None]
    ok = agreeing_pixels(render, alphas, r_o, a_o)
    outside = 1.0 - ok.double().mean().item()
    print(f"[fwd batches] {tag}: pixels outside the tolerance {outside:.2e}")
    assert outside <= MAX_OUTSIDE, (tag, outside)

    # hit lists
    n_hits = _check_hit_lists(rc, sc)
    assert (n_hits > 0) == bool((alphas > 0).any()), tag
    if name == "quadrant0":
        assert rc.hit_counts[1:4].abs().sum().item() == 0, (tag, rc.hit_counts[:4].tolist())
        blank = alphas[..., 0].clone()
        blank[:8, :8] = 0.0
        assert float(blank.abs().max()) == 0.0, tag

    # stale LDS: the same render after LDS was filled with NaNs, bit for bit (hit lists included)
    lib = load_library()
    check(lib.gsl_dev_poison_lds(0xFFFFFFFF, current_stream()), "gsl_dev_poison_lds")
    r2, a2 = rc.forward(*ins)
    torch.cuda.synchronize()
    assert torch.equal(r2, first[0]) and torch.equal(a2, first[1]), tag
    assert torch.equal(rc.hit_counts[:4 * rc.n_tiles], first[3][:4 * rc.n_tiles]), tag
    assert _check_hit_lists(rc, sc) == n_hits
    offs, counts = rc.offs.cpu().tolist(), rc.hit_counts.cpu().tolist()
    for t in range(rc.n_tiles):
        for q in range(4):
            a = 4 * offs[t] + q * (offs[t + 1] - offs[t])
            assert torch.equal(rc.hits[a:a + counts[4 * t + q]], first[2][a:a + counts[4 * t + q]]), (tag, t, q)

    # gradients on the agreeing pixels (the hit lists of the forward just run are what the backward walks)
    subsets = {"all": torch.arange(N)}
    for kind in ("random", "depth"):
        v, va = _upstream(kind, H, W, ok)
        ref, floor32 = _oracle_backward(name, opacity, kind, v, va)
        if kind == "depth":
            rc.forward(*ins)
        g = rc.backward(v.float().to(dev).contiguous(), va.float().to(dev).contiguous(), full=True)
        g = {k: (t.clone() if t is not None else None) for k, t in rc.grads_in_input_order(g).items()}
        torch.cuda.synchronize()
        rc.check_capacity()
        names = ("means", "scales", "opacities", "colors") if kind == "random" else ("means", "scales", "opacities")
        got = {k: g[k] for k in names}
        worst, counts_g, _ = compare_grads(got, {k: torch.from_numpy(ref["v_" + k]) for k in names}, subsets)
        err_v = rel_inf(g["viewmat"][:3], ref["v_viewmat"][:3])
        print(f"[fwd batches] {tag} upstream {kind}: v_viewmat {err_v:.2e} (float32 floor {floor32:.2e}), "
              + ", ".join(f"v_{k} {x:.2e}" for k, x in worst.items()) + f", outlier Gaussians {counts_g['all'][0]} of {N}")
        for k in names:
            assert torch.isfinite(g[k]).all(), (tag, kind, k)
        assert floor32 < FLOOR32_MAX, (tag, kind, floor32)
        assert err_v < _pose_bound(name, floor32), (tag, kind, err_v, floor32)
        assert not failing_subsets(counts_g), (tag, kind, counts_g, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("opacity", OPACITIES)
@pytest.mark.parametrize("name", TINY_SCENES)
def test_tiny_backward_on_the_same_scenes(name, opacity, monkeypatch):
    """k_tiny_bwd shares the compaction helper (slot numbers instead of byte offsets, back to front): a list of zero
    counts in three quadrants, and one that ends an entry after a batch boundary."""
    from gsplatloc_amd.context import RenderContext

    dev = torch.device("cuda")
    monkeypatch.setenv("GSLOC_BWD", "tiny")
    sc = _scene(name, opacity)
    N, W, H = sc["N"], sc["W"], sc["H"]
    want = _oracle_forward(name, opacity)
    rc = RenderContext(N, W, H, "RGB+ED", sh_degree=1, K_sh=4, device=dev, full_grads=True)
    ins = [t.to(dev).contiguous() for t in _oracle_inputs(sc)]
    assert rc.calibrate(*ins) == want["n_isects"] and rc.tiny
    render, alphas = rc.forward(*ins)
    ok = agreeing_pixels(render, alphas, torch.from_numpy(want["render"]), torch.from_numpy(want["alphas"])[..., None])
    assert 1.0 - ok.double().mean().item() <= MAX_OUTSIDE
    v, va = _upstream("random", H, W, ok)
    ref, floor32 = _oracle_backward(name, opacity, "random", v, va)
    g = rc.backward(v.float().to(dev).contiguous(), va.float().to(dev).contiguous(), full=True)
    g = {k: (t.clone() if t is not None else None) for k, t in rc.grads_in_input_order(g).items()}
    torch.cuda.synchronize()
    rc.check_capacity()
    assert not rc.tiny_overflowed()
    names = ("means", "scales", "opacities", "colors")
    worst, counts_g, _ = compare_grads({k: g[k] for k in names}, {k: torch.from_numpy(ref["v_" + k]) for k in names},
                                       {"all": torch.arange(N)})
    err_v = rel_inf(g["viewmat"][:3], ref["v_viewmat"][:3])
    print(f"[fwd batches] tiny {name} opacity {opacity}: v_viewmat {err_v:.2e} (float32 floor {floor32:.2e}), "
          + ", ".join(f"v_{k} {x:.2e}" for k, x in worst.items()))
    assert floor32 < FLOOR32_MAX and err_v < _pose_bound(name, floor32), (name, opacity, err_v, floor32)
    assert not failing_subsets(counts_g), (name, opacity, counts_g, worst)
