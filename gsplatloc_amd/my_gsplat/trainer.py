"""Pose tracker: the per-frame body of ``Runner.train``
(/root/reference/src/my_gsplat/gs_trainer_total.py:53-267) without the W&B / viewer plumbing.

Two engines, same arithmetic:
  * ``engine="autograd"`` -- the reference's loop verbatim: GSModel + CameraOptModule_quat_tans,
    losses from ``loss.py``, ``total_loss.backward()``, two Adam optimisers, ExponentialLR.
    Every rasterization call goes through the gsplat-compatible entry (fused HIP pipeline).
  * ``engine="context"``  -- same iteration on a preallocated ``RenderContext`` (no allocator
    traffic, no per-call size read-back, pose-only backward: the Gaussian gradients the reference
    computes and never consumes are skipped).
Pose errors: /root/reference/src/eval/utils.py:122-168.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional

import torch
from torch import Tensor

from ..context import RenderContext
from .loss import (compute_depth_loss, compute_normal_consistency_loss, compute_rgb_l1_loss, compute_silhouette_loss,
                   compute_ssim_loss)
from .model import CameraConfig, CameraOptModule_quat_tans, GsConfig, GSModel


def calculate_translation_error(estimated_pose: Tensor, true_pose: Tensor) -> float:
    """eval/utils.py:122-141."""
    return float(torch.norm(estimated_pose[:3, 3] - true_pose[:3, 3]))


def calculate_rotation_error(estimated_pose: Tensor, true_pose: Tensor) -> float:
    """eval/utils.py:144-168: rotation angle of R_est R_gt^T in degrees.  The reference takes
    acos((trace - 1) / 2), which float32 resolves only down to ~0.02 degrees; the same angle from
    |R_est - R_gt|_F^2 = 8 sin^2(theta / 2) is accurate at the 1e-3 degree level the tracker reaches
    (same formula as csrc/tracker.hip)."""
    d = estimated_pose[:3, :3] - true_pose[:3, :3]
    s = torch.sqrt((d * d).sum() * 0.125).clamp(max=1.0)
    return float(2.0 * torch.asin(s) * 180.0 / math.pi)


@dataclass
class TrackerConfig:
    """data/base.py:22-43 (OptimizationConfig) + gs_trainer_total.py:34."""
    max_steps: int = 1000
    depth_lambda: float = 0.8
    normal_lambda: float = 0.0
    # the photometric term the reference writes out and keeps commented (gs_trainer_total.py:111-123): it enters the
    # total as rgb_lambda * ((1 - ssim_lambda) * rgb_l1 + ssim_lambda * (1 - ssim)), beside the three weights above
    rgb_lambda: float = 0.0
    ssim_lambda: float = 0.5  # data/base.py:26
    early_stop: bool = True
    patience: int = 200
    min_step: int = 100  # "if step > 100" (gs_trainer_total.py:171)
    camera: CameraConfig = CameraConfig()
    gs: GsConfig = field(default_factory=GsConfig)


@dataclass
class TrackResult:
    losses: List[float] = field(default_factory=list)
    best_loss: float = float("inf")
    best_depth_loss: float = float("inf")
    best_silhouette_loss: float = float("inf")
    best_rgb_l1_loss: float = float("inf")  # the photometric term's two parts at the best step (rgb_lambda != 0 only)
    best_ssim_loss: float = float("inf")
    best_eT: float = float("inf")
    best_eR: float = float("inf")
    final_c2w: Optional[Tensor] = None
    steps: int = 0
    # the pose of the minimum-loss iterate (the one best_eT / best_eR were read from) and its step; no minimum was ever
    # recorded (best_step == -1: num_iters <= min_step + 1, or early_stop off): best_c2w is final_c2w
    best_c2w: Optional[Tensor] = None
    best_step: int = -1


class PoseTracker:
    def __init__(self, config: TrackerConfig = TrackerConfig(), engine: str = "autograd"):
        assert engine in ("autograd", "context")
        self.config = config
        self.engine = engine

    def tracking_loss(self, depths: Tensor, depths_gt: Tensor, K: Optional[Tensor] = None,
                      colors: Optional[Tensor] = None, pixels: Optional[Tensor] = None):
        """gs_trainer_total.py:105-150.  The normal-consistency term is the call the reference keeps commented
        out (:138-143) behind normal_lambda = 0 (data/base.py:28); it is evaluated only for a non-zero weight.  So is
        the photometric term (:111-123; rendered ``colors`` and the target image ``pixels``, both [1,H,W,3]): its two
        parts are left in ``self.last_photo`` = (rgb_l1, 1 - ssim), None when the weight is 0."""
        mask = (depths != 0).float()
        depth_loss = compute_depth_loss(depths * mask, depths_gt * mask, loss_type="l1")
        silhouette_loss = compute_silhouette_loss(depths * mask, depths_gt * mask, loss_type="l1")
        total = depth_loss * self.config.depth_lambda + silhouette_loss * (
            1 - self.config.depth_lambda - self.config.normal_lambda)
        if self.config.normal_lambda != 0.0:
            assert K is not None, "the normal-consistency term back-projects through K"
            normal_loss = compute_normal_consistency_loss((depths * mask)[0, :, :, 0], (depths_gt * mask)[0, :, :, 0],
                                                          K=K, loss_type="cosine")
            total = total + normal_loss * self.config.normal_lambda
        self.last_photo = None
        if self.config.rgb_lambda != 0.0:
            if pixels is None or colors is None:
                raise ValueError("rgb_lambda != 0: the photometric term needs the rendered colours and the target image "
                                 "(pixels)")
            rgb_l1 = compute_rgb_l1_loss(colors, pixels, mask)
            ssim_loss = compute_ssim_loss(colors, pixels, mask)
            lam = self.config.ssim_lambda
            total = total + self.config.rgb_lambda * ((1 - lam) * rgb_l1 + lam * ssim_loss)
            self.last_photo = (rgb_l1, ssim_loss)
        return total, depth_loss, silhouette_loss

    def track_frame(self, tar_points: Tensor, colors: Tensor, src_depth: Tensor, tar_c2w: Tensor, src_c2w: Tensor,
                    K: Tensor, width: int, height: int, scales: Optional[Tensor] = None,
                    verbose: bool = False, pixels: Optional[Tensor] = None) -> TrackResult:
        """One frame pair: Gaussians from the previous frame (``tar_points``), initial pose ``tar_c2w``,
        target depth ``src_depth`` [1,H,W,1], reference pose ``src_c2w`` for the error read-out; ``pixels``
        [1,H,W,3] in 0..1 is the target image of the photometric term (needed, and read, for rgb_lambda != 0 only)."""
        cfg = self.config
        if cfg.rgb_lambda != 0.0 and pixels is None:
            raise ValueError("rgb_lambda != 0: track_frame needs the target image (pixels)")
        max_steps = cfg.max_steps
        Ks = K.unsqueeze(0)
        gs_splats = GSModel(tar_points, colors, config=cfg.gs, scales=scales)
        camera_opt = CameraOptModule_quat_tans(tar_c2w, config=cfg.camera).to(tar_points.device)
        gamma = 0.2 ** (1.0 / max_steps)
        schedulers = [torch.optim.lr_scheduler.ExponentialLR(o, gamma=gamma) for o in camera_opt.optimizers]
        rc = None
        if self.engine == "context":
            rc = RenderContext(len(gs_splats), width, height, "RGB+ED", sh_degree=cfg.gs.sh_degree,
                               K_sh=(cfg.gs.sh_degree + 1) ** 2, device=tar_points.device,
                               near_plane=cfg.gs.near_plane, far_plane=cfg.gs.far_plane, full_grads=False)
            opac = torch.sigmoid(gs_splats.opacities).contiguous()
            sh = torch.cat([gs_splats.sh0, gs_splats.shN], 1).contiguous()
            statics = (gs_splats.means3d.contiguous(), gs_splats.quats.contiguous(), gs_splats.scales.contiguous(),
                       opac, sh)
            with torch.no_grad():
                rc.calibrate(*statics, torch.linalg.inv(camera_opt()).contiguous(), K.contiguous(), headroom=1.5)
        res = TrackResult()
        counter = 0
        for step in range(max_steps):
            camera_opt.optimizer_clean()
            cur_c2w = camera_opt()
            if rc is None:
                renders, alphas, _ = gs_splats(camtoworlds=cur_c2w.unsqueeze(0), Ks=Ks, width=width, height=height)
            else:
                viewmat = torch.linalg.inv(cur_c2w).contiguous()
                render, _ = rc.render_autograd(*statics, viewmat, K.contiguous())
                renders = render.unsqueeze(0)
            assert renders.shape[-1] == 4
            depths = renders[..., 3:4]
            total_loss, depth_loss, silhouette_loss = self.tracking_loss(depths, src_depth, K, renders[..., 0:3], pixels)
            total_loss.backward()
            with torch.no_grad():
                lv = total_loss.item()
                res.losses.append(lv)
                if cfg.early_stop:
                    eT = calculate_translation_error(cur_c2w, src_c2w)
                    eR = calculate_rotation_error(cur_c2w, src_c2w)
                    if step > cfg.min_step:
                        if lv < res.best_loss:
                            res.best_loss = lv
                            res.best_silhouette_loss = silhouette_loss.item()
                            res.best_depth_loss = depth_loss.item()
                            if self.last_photo is not None:
                                res.best_rgb_l1_loss, res.best_ssim_loss = (v.item() for v in self.last_photo)
                            res.best_eT, res.best_eR = eT, eR
                            res.best_c2w, res.best_step = cur_c2w.detach().clone(), step
                            counter = 0
                        else:
                            counter += 1
                    if verbose:
                        print(f"step {step} loss={lv:.8f} eT={eT:.3e} eR={eR:.3e}")
                res.steps = step + 1
                res.final_c2w = cur_c2w.detach().clone()
                if cfg.early_stop and counter >= cfg.patience:
                    break
            camera_opt.optimizer_step()
            for s in schedulers:
                s.step()
        if rc is not None:
            rc.check_capacity()
        if res.best_step == -1:
            res.best_c2w = res.final_c2w
        return res
