"""CPU: the photometric term (RGB L1 + SSIM).  The inputs of the GPU tests sit on no tie and the reference's own float32
evaluation stays well inside the kernels' bound; my_gsplat.loss mirrors the reference; PoseTracker and GraphTracker take
the term, and refuse what it cannot do with the reason in the message."""
import pytest
import torch

from tests import photo_ref as R


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("W,H", R.SHAPES)
def test_inputs_sit_on_no_tie_and_float32_reference_is_close(W, H, kind):
    colors, depth, pixels = R.photo_inputs(W, H, kind)
    ref = R.evaluate(colors, depth, pixels)
    R.assert_no_tie(ref, f"{W}x{H} {kind}")
    lo = R.evaluate(colors, depth, pixels, dtype=torch.float32)
    gerr, serr = R.grad_error(lo.grad, ref.grad), abs(lo.ssim - ref.ssim)
    print(f"[photo-ref] {W}x{H} {kind}: min |c-p| {ref.min_diff:.2e}, min variance {ref.min_var:.2e}, "
          f"float32 reference: gradient {gerr:.2e}, ssim {serr:.2e}")
    assert ref.min_diff >= R.MIN_DIFF and ref.min_var > 0.0
    assert 0.1 < ref.count / (W * H) < 1.0  # some pixels masked, not all
    assert gerr <= R.GUARD_GRAD and serr <= R.GUARD_SSIM


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("W,H", R.SHAPES)
def test_loss_mirrors_agree_with_the_reference(W, H, kind):
    from gsplatloc_amd.my_gsplat import compute_rgb_l1_loss, compute_ssim_loss
    colors, depth, pixels = R.photo_inputs(W, H, kind)
    ref = R.evaluate(colors, depth, pixels)
    col = colors.double()[None].clone().requires_grad_()
    mask = (depth != 0).double()[None, ..., None]
    l1 = compute_rgb_l1_loss(col, pixels.double()[None], mask)
    ssim_loss = compute_ssim_loss(col, pixels.double()[None], mask)
    total = R.RGB_LAMBDA * ((1 - R.SSIM_LAMBDA) * l1 + R.SSIM_LAMBDA * ssim_loss)
    total.backward()
    assert abs(float(l1.detach()) - ref.l1) <= 1e-10 and abs(1 - float(ssim_loss.detach()) - ref.ssim) <= 1e-10
    assert abs(float(total.detach()) - ref.total) <= 1e-10
    assert float((col.grad[0] - ref.grad).abs().max()) <= 1e-10
    # [H,W,3] images and an [H,W] mask are taken as well
    assert float(compute_ssim_loss(colors.double(), pixels.double(), depth != 0)) == float(ssim_loss.detach())


def test_identical_images_have_ssim_one_and_no_photometric_loss():
    from gsplatloc_amd.my_gsplat import compute_rgb_l1_loss, compute_ssim_loss
    colors, depth, _ = R.photo_inputs(27, 21, "noise")
    ref = R.evaluate(colors, depth, colors)
    assert abs(ref.ssim - 1.0) <= 1e-12 and ref.l1 == 0.0 and abs(ref.total) <= 1e-12
    mask = (depth != 0).double()[None, ..., None]
    assert float(compute_rgb_l1_loss(colors.double()[None], colors.double()[None], mask)) == 0.0
    assert abs(float(compute_ssim_loss(colors.double()[None], colors.double()[None], mask))) <= 1e-12


def test_images_below_the_window_are_refused():
    from gsplatloc_amd._lib import load_library
    from gsplatloc_amd.my_gsplat import compute_ssim_loss
    colors, depth, pixels = R.photo_inputs(16, 16, "noise")
    with pytest.raises(ValueError, match="11x11"):
        compute_ssim_loss(colors[:10][None], pixels[:10][None], (depth[:10] != 0)[None, ..., None])
    with pytest.raises(ValueError):
        R.evaluate(colors[:, :10], depth[:, :10], pixels[:, :10])
    # ... and by the library, on the host, before any launch: a side below 11, another channel count, null pointers, a
    # short workspace (the pointers are never followed)
    lib = load_library()
    assert lib.gsl_photo_ws_bytes(16, 10) == 0 and lib.gsl_photo_ws_bytes(10, 16) == 0
    n = lib.gsl_photo_ws_bytes(27, 21)
    assert n >= 9 * 4 * 17 * 11 + 3 * 4 * 4
    assert lib.gsl_photo_loss(64, 4, 64, 16, 10, 0.2, 0.5, 64, 64, 64, 1 << 20, None) == -1
    assert lib.gsl_photo_loss(64, 4, 64, 10, 16, 0.2, 0.5, 64, 64, 64, 1 << 20, None) == -1
    assert lib.gsl_photo_loss(64, 3, 64, 27, 21, 0.2, 0.5, 64, 64, 64, 1 << 20, None) == -1
    for k in range(5):
        args = [64, 4, 64, 27, 21, 0.2, 0.5, 64, 64, 64, 1 << 20, None]
        args[(0, 2, 7, 8, 9)[k]] = None
        assert lib.gsl_photo_loss(*args) == -1, k
    assert lib.gsl_photo_loss(64, 4, 64, 27, 21, 0.2, 0.5, 64, 64, 64, n - 1, None) == -2


def test_tracking_loss_without_a_weight_ignores_the_image():
    import gsplatloc_amd.my_gsplat as M
    colors, depth, pixels = R.photo_inputs(27, 21, "near")
    g = torch.Generator().manual_seed(3)
    depths, target = depth[None, ..., None], (depth + 0.1 * torch.rand(21, 27, generator=g))[None, ..., None]
    pt = M.PoseTracker(M.TrackerConfig())
    plain = pt.tracking_loss(depths, target)
    given = pt.tracking_loss(depths, target, None, colors[None], pixels[None])
    assert pt.last_photo is None
    for a, b in zip(plain, given):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # with a weight the term is added as rgb_lambda * ((1 - ssim_lambda) l1 + ssim_lambda (1 - ssim)) ...
    cfg = M.TrackerConfig(rgb_lambda=R.RGB_LAMBDA, ssim_lambda=R.SSIM_LAMBDA)
    pw = M.PoseTracker(cfg)
    total = pw.tracking_loss(depths.double(), target.double(), None, colors.double()[None], pixels.double()[None])[0]
    ref = R.evaluate(colors, depth, pixels)
    assert abs(float(total) - float(plain[0].double()) - ref.total) <= 1e-7
    assert abs(float(pw.last_photo[0]) - ref.l1) <= 1e-10 and abs(1 - float(pw.last_photo[1]) - ref.ssim) <= 1e-10
    # ... and needs the image
    with pytest.raises(ValueError, match="pixels"):
        pw.tracking_loss(depths, target)
    with pytest.raises(ValueError, match="pixels"):
        pw.track_frame(torch.zeros(4, 3), torch.zeros(4, 3), target, torch.eye(4), torch.eye(4), torch.eye(3), 27, 21)


def test_defaults_keep_the_term_off():
    import gsplatloc_amd.my_gsplat as M
    cfg, res = M.TrackerConfig(), M.trainer.TrackResult()
    assert cfg.rgb_lambda == 0.0 and cfg.ssim_lambda == 0.5
    assert res.best_rgb_l1_loss == float("inf") and res.best_ssim_loss == float("inf")


def test_graph_tracker_refusals(monkeypatch):
    import gsplatloc_amd.graph_tracker as GT
    from gsplatloc_amd.my_gsplat import TrackerConfig
    cfg = TrackerConfig(max_steps=5, rgb_lambda=0.2)
    with pytest.raises(ValueError, match="RGB\\+ED"):
        GT.GraphTracker(100, 64, 48, cfg, device="cpu", render_mode="ED")
    with pytest.raises(NotImplementedError, match="5-row halo"):
        GT.GraphTracker(100, 64, 48, cfg, device="cpu", rows=(0, 2))
    with pytest.raises(NotImplementedError, match="fourth"):
        GT.GraphTracker(100, 64, 48, cfg, device="cpu", group=object())
    with pytest.raises(ValueError, match="11x11"):
        GT.GraphTracker(100, 64, 10, cfg, device="cpu")

    class _Stream:
        def __init__(self, *a, **k):
            pass

    monkeypatch.setattr(torch.cuda, "Stream", _Stream)
    gt = GT.GraphTracker(100, 64, 48, cfg, device="cpu", use_graph=False)
    assert gt.pixels.shape == (48, 64, 3) and gt.photo_ws.numel() == gt.lib.gsl_photo_ws_bytes(64, 48)
    with pytest.raises(ValueError, match="pixels"):  # refused before anything is copied or launched
        gt.load_frame(torch.zeros(100, 3), torch.zeros(100, 3), torch.zeros(100, 3), torch.zeros(48, 64), torch.eye(4),
                      torch.eye(4), torch.eye(3))
    # without a weight nothing of the term is allocated, whatever the mode
    off = GT.GraphTracker(100, 64, 48, TrackerConfig(max_steps=5), device="cpu", use_graph=False, render_mode="ED")
    assert off.pixels is None and off.photo_ws is None and off.photo_sums is None


def test_graph_tracker_iteration_with_the_term_marshals_every_call(monkeypatch):
    """load_frame() and one _iteration() on host tensors with rgb_lambda != 0: the launch order of the term (depth
    losses, photometric loss, backward reading the gradient as given, photometric pose step), every call reached and none
    rejected by ctypes or by argument validation (the status check is relaxed to 'refused by the HIP runtime')."""
    import gsplatloc_amd.graph_tracker as GT
    import gsplatloc_amd.stages as ST
    from gsplatloc_amd.my_gsplat import TrackerConfig
    from gsplatloc_amd.my_gsplat.geometry import depth_to_points
    from gsplatloc_amd.synthetic import frame_pair

    calls = []

    def refused(status, what):
        calls.append(what)
        assert status == -3, (what, status)

    class _Stream:
        def __init__(self, *a, **k):
            pass

    for mod in (ST, GT):
        monkeypatch.setattr(mod, "current_stream", lambda: None)
        monkeypatch.setattr(mod, "check", refused)
    monkeypatch.setattr(torch.cuda, "Stream", _Stream)
    W, H = 64, 48
    fp = frame_pair(W, H, rot_deg=0.3, trans=0.01)
    pts = depth_to_points(fp["depth0"], fp["K"])
    gt = GT.GraphTracker(pts.shape[0], W, H, TrackerConfig(max_steps=5, rgb_lambda=0.2), device="cpu", use_graph=False)
    gt.load_frame(pts, fp["rgb"], torch.full((pts.shape[0], 3), 0.01), fp["depth1"], fp["c2w0"], fp["c2w1"], fp["K"],
                  pixels=torch.rand(1, H, W, 3))
    assert gt.pose_f[34:36].tolist() == [float("inf")] * 2
    del calls[:]
    gt._iteration()
    assert gt.rc.tiny  # the backward that could compute the depth loss itself: not chosen with a colour gradient
    assert calls == ["gsl_fused_project", "gsl_fused_raster_fwd", "gsl_tracking_loss", "gsl_photo_loss",
                     "gsl_tiny_raster_bwd", "gsl_fused_project_bwd", "gsl_pose_step_photo"]
