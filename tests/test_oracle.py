"""Pin the oracle: vectorised autograd restatement vs sequential hand-derived
restatement vs central finite differences (float64), plus invariants.

PARITY UNPINNED: the reference holds no golden vector for this path (SURVEY.md
8c); these checks are what stands in for it.
"""
import math

import numpy as np
import pytest
import torch

from oracle import gsplat_oracle as G
from oracle import sequential as S
from oracle import tracker_oracle as T
from tests.scenes import random_scene, sh_from_rgb, small_pose


def _stage(sc, c2w, D=2, aniso_colors=True, seed=3):
    W, H = sc["W"], sc["H"]
    V = torch.linalg.inv(c2w)[None]
    radii, m2, dep, con, _ = G.fully_fused_projection(sc["means"], sc["quats"], sc["scales"], V, sc["K"][None], W, H)
    tw, th = math.ceil(W / 16), math.ceil(H / 16)
    _, ids, fl = G.isect_tiles(m2, radii, dep, 16, tw, th)
    offs = G.isect_offset_encode(ids, 1, tw, th)
    g = torch.Generator().manual_seed(seed)
    cols = torch.rand(1, sc["means"].shape[0], D, generator=g, dtype=torch.float64)
    return radii, m2, dep, con, ids, fl, offs, cols, tw, th


@pytest.mark.parametrize("opacity", [None, (0.2, 0.9)])
def test_composite_sequential_matches_vectorised(opacity):
    sc = random_scene(150, 48, 32, sigma_px=2.0, opacity=opacity)
    radii, m2, dep, con, ids, fl, offs, cols, tw, th = _stage(sc, small_pose(0.0, 0.0))
    opa = sc["opacities"][None]
    m2r, conr, colr, opar = (x.clone().requires_grad_() for x in (m2, con, cols, opa))
    rc, ra = G.rasterize_to_pixels(m2r, conr, colr, opar, 48, 32, 16, offs, fl)
    out, al, last = S.composite_fwd(m2[0].numpy(), con[0].numpy(), cols[0].numpy(), opa[0].numpy(), 48, 32, 16,
                                    offs[0].numpy(), fl.numpy())
    np.testing.assert_allclose(rc[0].detach().numpy(), out, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(ra[0, ..., 0].detach().numpy(), al, rtol=1e-12, atol=1e-13)
    assert (al >= 0).all() and (al < 1).all()
    g = torch.Generator().manual_seed(1)
    v_out = torch.randn(rc.shape, generator=g, dtype=torch.float64)
    v_al = torch.randn(ra.shape, generator=g, dtype=torch.float64)
    (rc * v_out).sum().add((ra * v_al).sum()).backward()
    vm, vc, vcol, vo = S.composite_bwd(m2[0].numpy(), con[0].numpy(), cols[0].numpy(), opa[0].numpy(), 48, 32, 16,
                                       offs[0].numpy(), fl.numpy(), al, last, v_out[0].numpy(), v_al[0, ..., 0].numpy())
    np.testing.assert_allclose(m2r.grad[0].numpy(), vm, rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(conr.grad[0].numpy(), vc, rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(colr.grad[0].numpy(), vcol, rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(opar.grad[0].numpy(), vo, rtol=1e-9, atol=1e-11)


def test_projection_vjp_matches_autograd():
    sc = random_scene(60, 64, 48, sigma_px=1.5, aniso=True)
    c2w = small_pose(3.0, 0.05)
    V = torch.linalg.inv(c2w)[None].clone().requires_grad_()
    means, quats, scales = (sc[k].clone().requires_grad_() for k in ("means", "quats", "scales"))
    radii, m2, dep, con, _ = G.fully_fused_projection(means, quats, scales, V, sc["K"][None], 64, 48)
    g = torch.Generator().manual_seed(5)
    vm2, vdep, vcon = (torch.randn(x.shape, generator=g, dtype=torch.float64) for x in (m2, dep, con))
    ((m2 * vm2).sum() + (dep * vdep).sum() + (con * vcon).sum()).backward()
    vR = np.zeros((3, 3))
    vt = np.zeros(3)
    for i in range(60):
        if radii[0, i] <= 0:
            assert means.grad[i].abs().max() == 0
            continue
        v_mean, v_S, v_R, v_t = S.project_bwd_one(
            sc["means"][i].numpy(), sc["quats"][i].numpy(), sc["scales"][i].numpy(), V[0].detach().numpy(),
            sc["K"].numpy(), 64, 48, 0.3, vm2[0, i].numpy(), float(vdep[0, i]), vcon[0, i].numpy())
        v_q, v_s = S.covar_to_quat_scale_vjp(sc["quats"][i].numpy(), sc["scales"][i].numpy(), v_S)
        np.testing.assert_allclose(means.grad[i].numpy(), v_mean, rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(quats.grad[i].numpy(), v_q, rtol=1e-7, atol=1e-9)
        np.testing.assert_allclose(scales.grad[i].numpy(), v_s, rtol=1e-7, atol=1e-9)
        vR += v_R
        vt += v_t
    np.testing.assert_allclose(V.grad[0, :3, :3].numpy(), vR, rtol=1e-8, atol=1e-9)
    np.testing.assert_allclose(V.grad[0, :3, 3].numpy(), vt, rtol=1e-8, atol=1e-9)


def _loss_of_pose(sc, sh, q, t, gt):
    c2w = T.camera_forward(q, t)
    opac = sc["opacities"]
    r, a, _ = T.gs_forward(sc["means"], sc["quats"], sc["scales"], opac, sh, c2w, sc["K"], sc["W"], sc["H"])
    total, dl, sl = T.tracking_loss(r[..., 3:4], gt)
    return total


def test_pose_gradient_vs_finite_differences():
    """d(0.8*L1 + 0.2*Sobel-L1)/d(quat, t) by autograd vs central differences, float64."""
    sc = random_scene(400, 64, 48, sigma_px=2.5, opacity=(0.3, 0.8))
    sh = sh_from_rgb(sc["rgbs"])
    with torch.no_grad():
        gt, _, _ = T.gs_forward(sc["means"], sc["quats"], sc["scales"], sc["opacities"], sh, small_pose(0, 0), sc["K"], 64, 48)
        gt = gt[..., 3:4]
    c2w0 = small_pose(0.4, 0.01)
    q = T.rotation_matrix_to_quaternion(c2w0[:3, :3].contiguous()).clone().requires_grad_()
    t = c2w0[:3, 3].clone().requires_grad_()
    L = _loss_of_pose(sc, sh, q, t, gt)
    L.backward()
    an = torch.cat([q.grad, t.grad]).numpy()
    fd = np.zeros(7)
    eps = 1e-6
    for k in range(7):
        d = torch.zeros(7, dtype=torch.float64)
        d[k] = eps
        with torch.no_grad():
            lp = _loss_of_pose(sc, sh, q + d[:4], t + d[4:], gt)
            lm = _loss_of_pose(sc, sh, q - d[:4], t - d[4:], gt)
        fd[k] = float(lp - lm) / (2 * eps)
    scale = np.abs(an).max()
    assert scale > 1e-6
    np.testing.assert_allclose(an, fd, rtol=2e-4, atol=2e-5 * scale)


def test_binning_invariants():
    sc = random_scene(500, 100, 70, sigma_px=3.0)
    radii, m2, dep, con, ids, fl, offs, cols, tw, th = _stage(sc, small_pose(1.0, 0.02))
    tpg, ids_u, fl_u = G.isect_tiles(m2, radii, dep, 16, tw, th, sort=False)
    assert int(tpg.sum()) == ids.numel() == fl.numel()
    assert (ids[1:] >= ids[:-1]).all()
    assert sorted(ids_u.tolist()) == ids.tolist()
    assert offs.shape == (1, th, tw)
    o = offs.reshape(-1).tolist() + [ids.numel()]
    assert all(o[i] <= o[i + 1] for i in range(len(o) - 1))
    tile_of = (ids >> 32).tolist()
    for t in range(tw * th):
        assert all(x == t for x in tile_of[o[t]:o[t + 1]])
    # zero-radius Gaussians never appear
    assert (radii[0][fl.long()] > 0).all()


def test_expected_depth_of_frontoparallel_plane():
    """ED depth of a dense fronto-parallel plane equals the plane depth."""
    W, H, z0 = 48, 32, 2.0
    K = torch.tensor([[40.0, 0, 23.5], [0, 40.0, 15.5], [0, 0, 1]], dtype=torch.float64)
    depth = torch.full((H, W), z0, dtype=torch.float64)
    pts = T.depth_to_points(depth, K)
    N = pts.shape[0]
    scales = torch.full((N, 3), 0.02, dtype=torch.float64)
    quats = torch.tensor([1.0, 0, 0, 0], dtype=torch.float64).repeat(N, 1)
    sh = torch.zeros(N, 4, 3, dtype=torch.float64)
    r, a, _ = T.gs_forward(pts, quats, scales, torch.ones(N, dtype=torch.float64), sh, torch.eye(4, dtype=torch.float64), K, W, H)
    d = r[0, 2:-2, 2:-2, 3]
    assert torch.allclose(d, torch.full_like(d, z0), rtol=1e-9)
    assert (a[0, 2:-2, 2:-2] > 0.9).all()


def test_kornia_restatements():
    q = torch.tensor([0.9, 0.1, -0.3, 0.2], dtype=torch.float64)
    R = T.quaternion_to_rotation_matrix(q)
    assert torch.allclose(R @ R.T, torch.eye(3, dtype=torch.float64), atol=1e-12)
    assert torch.allclose(torch.det(R), torch.tensor(1.0, dtype=torch.float64))
    assert torch.allclose(R, G.quat_to_rotmat(q), atol=1e-12)
    q2 = T.rotation_matrix_to_quaternion(R)
    assert torch.allclose(q2, q / q.norm(), atol=1e-7)
    x = torch.arange(20.0, dtype=torch.float64).reshape(1, 1, 4, 5)
    s = T.sobel(x)  # d/dx = 1, d/dy = 5 in the interior, kernel normalised by 8
    assert torch.allclose(s[0, 0, 1:-1, 1:-1], torch.full((2, 3), math.sqrt(1 + 25 + 1e-6), dtype=torch.float64))


def test_zero_pose_gradient_at_gt_and_convergence():
    sc = random_scene(600, 64, 48, sigma_px=2.5, opacity=(0.5, 0.9), dtype=torch.float64)
    sh = sh_from_rgb(sc["rgbs"])
    I4 = torch.eye(4, dtype=torch.float64)
    with torch.no_grad():
        gt, _, _ = T.gs_forward(sc["means"], sc["quats"], sc["scales"], sc["opacities"], sh, I4, sc["K"], 64, 48)
    q = torch.tensor([1.0, 0, 0, 0], dtype=torch.float64, requires_grad=True)
    t = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    L = _loss_of_pose(sc, sh, q, t, gt[..., 3:4])
    L.backward()
    assert float(L.detach()) < 1e-12 or q.grad.abs().max() < 1e-6
    res = T.track_frame(sc["means"], sc["scales"], sc["rgbs"], gt[..., 3:4], sc["K"], 64, 48,
                        init_c2w=small_pose(0.3, 0.01), gt_c2w=I4, max_steps=60, min_step=5)
    assert min(res.losses) < 0.9 * res.losses[0]


@pytest.mark.parametrize("mode,sh_degree,aa", [("RGB+ED", 1, False), ("RGB", None, True), ("D", None, False),
                                               ("RGB+D", 3, True), ("ED", None, False)])
def test_half_record_oracle_without_rounding_is_the_oracle(mode, sh_degree, aa):
    """tests/grad_paths.oracle_render (the oracle's stages, with the fp16 record's rounding when asked) gives
    G.rasterization's render, alpha and gradients bit for bit when it does not round, and rounding moves them."""
    from tests.grad_paths import oracle_render

    sc = random_scene(300, 40, 28, seed=3, sigma_px=1.5, aniso=True, opacity=(0.2, 0.9))
    g = torch.Generator().manual_seed(5)
    colors = torch.randn(300, (sh_degree + 1) ** 2, 3, generator=g, dtype=torch.float64) if sh_degree else sc["rgbs"]
    V = torch.linalg.inv(small_pose(1.0, 0.02))
    outs = []
    for which in ("oracle", "plain", "half"):
        ins = [t.clone().requires_grad_() for t in (sc["means"], sc["quats"], sc["scales"], sc["opacities"], colors, V)]
        if which == "oracle":
            r, a, _ = G.rasterization(*ins[:5], ins[5][None], sc["K"][None], 40, 28, sh_degree=sh_degree,
                                      render_mode=mode, rasterize_mode="antialiased" if aa else "classic")
            r, a = r[0], a[0]
        else:
            r, a = oracle_render(*ins, sc["K"], 40, 28, mode, sh_degree=sh_degree, antialiased=aa, half=which == "half")
        (r.sum() + a.sum()).backward()
        outs.append([r.detach(), a.detach()] + [t.grad for t in ins])
    for x, y in zip(outs[0], outs[1]):
        assert (x is None and y is None) or torch.equal(x, y)
    assert not torch.equal(outs[0][0], outs[2][0])

