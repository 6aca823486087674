"""GPU: the photometric term end to end -- the device loop (gsl_tracking_loss, gsl_photo_loss, backward,
gsl_pose_step_photo, as a HIP graph or launch by launch) against the PyTorch loop with the same weights, on the 160x120
frame pair of test_gpu_tracker.py with point colours that vary smoothly over the image, so that the photometric
gradient means something."""
import functools
import math

import pytest
import torch

from gsplatloc_amd.synthetic import frame_pair
from oracle import tracker_oracle as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
STEPS = 30


def _smooth_colours(W, H):
    """[H*W,3] in [0.1, 0.9]: 0.5 + 0.4 sin of the pixel position, another direction and phase per channel"""
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    ch = [0.5 + 0.4 * torch.sin(a * u + b * v + c) for a, b, c in ((0.11, 0.03, 0.0), (0.02, 0.13, 1.0), (0.07, -0.09, 2.0))]
    return torch.stack(ch, -1).reshape(H * W, 3)


@functools.lru_cache(maxsize=None)
def _setup(W=160, H=120):
    """The frame pair, its target depth and target image, and the PyTorch loop's result: computed once, never modified."""
    import gsplatloc_amd as A
    import gsplatloc_amd.my_gsplat as M
    from gsplatloc_amd.my_gsplat.utils import rgb_to_sh
    fp = frame_pair(W, H, rot_deg=0.3, trans=0.01)
    K = fp["K"]
    pts0, pts1 = T.depth_to_points(fp["depth0"], K), T.depth_to_points(fp["depth1"], K)
    scales0, scales1 = T.init_gs_scales(pts0, as_coded=True), T.init_gs_scales(pts1, as_coded=True)
    rgb = _smooth_colours(W, H)
    # target: the "RGB+ED" render of the source cloud from the identity pose -- depth in channel 3, image in 0..2
    n = pts1.shape[0]
    quats = torch.tensor([1.0, 0.0, 0.0, 0.0]).repeat(n, 1)
    sh = torch.zeros(n, 4, 3)
    sh[:, 0] = rgb_to_sh(rgb)
    with torch.no_grad():
        render, _, _ = A.rasterization(means=pts1.to(DEV), quats=quats.to(DEV), scales=scales1.to(DEV),
                                       opacities=torch.ones(n, device=DEV), colors=sh.to(DEV), sh_degree=1,
                                       viewmats=torch.eye(4, device=DEV)[None], Ks=K[None].to(DEV), width=W, height=H,
                                       far_plane=1e10, near_plane=1e-2, render_mode="RGB+ED", rasterize_mode="classic",
                                       packed=False)
    src_depth = render[0, :, :, 3][None, ..., None].contiguous()
    pixels = render[0, :, :, 0:3][None].clamp(0.0, 1.0).contiguous()
    frame = (pts0.to(DEV), rgb.to(DEV), scales0.to(DEV), src_depth, fp["c2w0"].to(DEV), fp["c2w1"].to(DEV), K.to(DEV))
    cfg = M.TrackerConfig(max_steps=STEPS, min_step=5, patience=1000, rgb_lambda=0.2)
    pts, col, sc, depth, c0, c1, Kd = frame
    ref = M.PoseTracker(cfg, engine="context").track_frame(pts, col, depth, c0, c1, Kd, W, H, scales=sc, pixels=pixels)
    return M, W, H, frame, pixels, cfg, ref


@pytest.mark.parametrize("use_graph", [False, True])
def test_graph_tracker_with_the_photometric_term_follows_the_pose_tracker(use_graph):
    M, W, H, frame, pixels, cfg, ref = _setup()
    from gsplatloc_amd.graph_tracker import GraphTracker
    gt = GraphTracker(frame[0].shape[0], W, H, cfg, device=DEV, use_graph=use_graph, poll=10)
    gt.load_frame(*frame, pixels=pixels)
    res = gt.run()
    assert res.steps == ref.steps == STEPS
    lg, lr = torch.tensor(res.losses, dtype=torch.float64), torch.tensor(ref.losses, dtype=torch.float64)
    first, traj = abs(float(lg[0] - lr[0])) / float(lr[0]), float(((lg - lr).abs() / lr).max())
    e_l1 = abs(res.best_rgb_l1_loss - ref.best_rgb_l1_loss) / ref.best_rgb_l1_loss
    e_ss = abs(res.best_ssim_loss - ref.best_ssim_loss) / ref.best_ssim_loss
    print(f"[parity] tracker with photometric term (graph={use_graph}): loss0 rel {first:.1e}, trajectory rel {traj:.1e}, "
          f"best rgb l1 {res.best_rgb_l1_loss:.4e} rel {e_l1:.1e}, best 1-ssim {res.best_ssim_loss:.4e} rel {e_ss:.1e}, "
          f"loss {float(lg[0]):.4e} -> {float(lg[-1]):.4e}")
    assert first < 2e-5
    assert traj < 5e-3  # Adam amplifies float32 differences of the first updates (the bound of the normal-term test)
    assert math.isfinite(res.best_rgb_l1_loss) and math.isfinite(res.best_ssim_loss)
    assert math.isfinite(ref.best_rgb_l1_loss) and math.isfinite(ref.best_ssim_loss)
    assert e_l1 < 2e-3 and e_ss < 2e-3
    # a second frame on the same tracker (buffers and graph reused; the gradient buffer still holds the last iteration's)
    gt.load_frame(*frame, pixels=pixels)
    res2 = gt.run()
    assert torch.allclose(torch.tensor(res2.losses, dtype=torch.float64), lg, rtol=1e-4)
    assert res2.best_rgb_l1_loss == pytest.approx(res.best_rgb_l1_loss, rel=1e-4)


def test_graph_tracker_without_a_weight_ignores_the_image():
    M, W, H, frame, pixels, _, _ = _setup()
    from gsplatloc_amd.graph_tracker import GraphTracker
    cfg = M.TrackerConfig(max_steps=12, min_step=3, patience=1000)
    runs = []
    for px in (None, pixels):
        gt = GraphTracker(frame[0].shape[0], W, H, cfg, device=DEV, poll=6)
        gt.load_frame(*frame, pixels=px)
        runs.append(gt.run())
    assert runs[0].steps == runs[1].steps == 12
    assert runs[0].losses == runs[1].losses  # bit for bit: floats read back from the same device buffer
    assert runs[1].best_rgb_l1_loss == float("inf") and runs[1].best_ssim_loss == float("inf")
    assert torch.equal(runs[0].final_c2w, runs[1].final_c2w)
