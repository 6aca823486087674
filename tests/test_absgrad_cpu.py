"""absgrad without a GPU: the two C entry points reject bad arguments on the host, the kernel file compiles for gfx950
without scratch, and the Python paths make the right calls in the right order on host tensors (every launch refused by
the HIP runtime, as in test_marshalling_cpu.py)."""
import os
import re
import subprocess

import pytest
import torch

from gsplatloc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gsplatloc_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="host-pointer calls: only meaningful without a GPU")


def test_entries_are_declared_and_bound():
    assert {"gsl_fused_absgrad", "gsl_rasterize_absgrad"} <= set(_lib.exported_symbols())
    lib = _lib.load_library()
    assert hasattr(lib, "gsl_fused_absgrad") and hasattr(lib, "gsl_rasterize_absgrad")


def test_bad_arguments_are_rejected_without_a_gpu():
    lib = _lib.load_library()
    buf = torch.zeros(64)
    p = buf.data_ptr()
    W, H, tw, th = 64, 48, 4, 3

    def fused(channels=4, ed=1, cap=10, q0=p, q2=p, hits=None, counts=None, absgrad=p, w=W, t_w=tw):
        # Q0, Q1, Q2, channels, ed, width, height, tile_w, tile_h, tile_offsets, flatten_ids, capacity, render, alphas,
        # last_ids, v_render, v_alphas, isect_hits, isect_hit_counts, absgrad, stream
        return lib.gsl_fused_absgrad(q0, p, q2, channels, ed, w, H, t_w, th, p, p, cap, p, p, p, p, p, hits, counts,
                                     absgrad, None)

    assert fused(channels=2) == -1
    assert fused(channels=3, ed=1) == -1      # "ED" has a depth channel
    assert fused(q0=None) == -1
    assert fused(q2=None) == -1               # colour records for 3 / 4 channels
    assert fused(absgrad=None) == -1
    assert fused(hits=p) == -1                # hit lists and their lengths go together
    assert fused(w=65) == -1                  # more pixels than tiles
    assert fused(cap=-1) == -1
    assert fused(cap=0) == 0                  # nothing to walk: no launch

    def staged(channels=3, tile_size=16, means=p, absgrad=p, cap=10, bg=None):
        # means2d, conics, colors, opacities, backgrounds, channels, width, height, tile_size, tile_w, tile_h,
        # tile_offsets, flatten_ids, capacity, render_alphas, last_ids, t_final, v_render_colors, v_render_alphas, absgrad,
        # stream
        return lib.gsl_rasterize_absgrad(means, p, p, p, bg, channels, W, H, tile_size, tw, th, p, p, cap, p, p, None, p, p,
                                         absgrad, None)

    assert staged(tile_size=8) == -1
    assert staged(channels=7) == -1
    assert staged(channels=33) == -1
    assert staged(means=None) == -1
    assert staged(absgrad=None) == -1
    assert staged(cap=0) == 0


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_absgrad_kernels_do_not_spill():
    cmd = [HIPCC, "-O3", "-std=c++17", "-fno-slp-vectorize", "--offload-arch=gfx950", "--cuda-device-only", "-c",
           "absgrad.hip", "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC, timeout=900)
    assert res.returncode == 0, res.stderr[-2000:]
    out, cur = {}, None
    for line in res.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {}) if "k_absgrad" in m.group(1) else None
            continue
        m = re.search(r"remark:\s+(VGPRs|LDS Size \[bytes/block\]|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split(" ")[0]] = int(m.group(2))
    # fused: channels 1 (plain, ED), 3, 4 (plain, ED); staged: 1, 2, 3, 4, 5, 8, 16, 32
    assert len(out) == 13, sorted(out)
    for k, v in out.items():
        assert v["ScratchSize"] == 0 and v["LDS"] <= 16 * 1024, (k, v)


def _scene(N, W, H):
    from gsplatloc_amd.synthetic import perturbed_pose, random_scene

    sc = random_scene(N, W, H, sigma_px=1.0)
    V = torch.linalg.inv(perturbed_pose()).contiguous()
    return sc, V


@no_gpu
@pytest.mark.parametrize("mode,sh_degree", [("RGB+ED", 1), ("ED", None), ("RGB", None)])
def test_fused_absgrad_nodes_marshal(mode, sh_degree, monkeypatch):
    """The two autograd nodes of rendering.rasterization(absgrad=True) on the fused path, forward and backward."""
    import gsplatloc_amd.fused as F
    import gsplatloc_amd.stages as ST

    calls = []

    def refused(status, what):  # 0: nothing to launch (no intersections); -3: launch refused; never a rejected argument
        calls.append(what)
        assert status in (0, -3), (what, status)

    monkeypatch.setattr(ST, "check", refused)
    monkeypatch.setattr(ST, "current_stream", lambda: None)
    monkeypatch.setattr(torch, "empty", torch.zeros)  # the intersection count is read back from an output buffer
    N, W, H = 300, 64, 48
    sc, V = _scene(N, W, H)
    colors = sc["sh"] if sh_degree is not None else torch.rand(N, 3)
    ins = [sc[k].clone().requires_grad_() for k in ("means", "quats", "scales", "opacities")]
    col = colors.clone().requires_grad_()
    V = V.requires_grad_()
    cfg = F.FusedCfg(width=W, height=H, sh_degree=-1 if sh_degree is None else sh_degree, mode=mode, eps2d=0.3,
                     near_plane=0.01, far_plane=1e10, radius_clip=0.0, antialiased=False, ty0=0, ty1=3,
                     want_isect_ids=True)
    render, alphas, means2d, state = F.fused_absgrad_apply(*ins, col, V, sc["K"].contiguous(), cfg)
    assert render.shape == (H, W, F._MODES[mode][0]) and alphas.shape == (H, W, 1)
    assert means2d.shape == (1, N, 2) and means2d.requires_grad and means2d.grad_fn is not None
    means2d.retain_grad()
    (render.sum() + alphas.sum()).backward()
    assert calls == ["gsl_fused_project", "gsl_fused_bin", "gsl_fused_raster_fwd", "gsl_fused_raster_bwd",
                     "gsl_fused_absgrad", "gsl_fused_project_bwd"]
    assert means2d.absgrad.shape == (1, N, 2) and means2d.absgrad.dtype == torch.float32
    assert means2d.grad is not None and means2d.grad.shape == (1, N, 2)
    assert V.grad is not None and V.grad.shape == (4, 4) and ins[0].grad.shape == (N, 3)
    assert (col.grad is not None) == mode.startswith("RGB")


@no_gpu
def test_fused_absgrad_nodes_under_no_grad(monkeypatch):
    import gsplatloc_amd.fused as F
    import gsplatloc_amd.stages as ST

    monkeypatch.setattr(ST, "check", lambda status, what: None)
    monkeypatch.setattr(ST, "current_stream", lambda: None)
    monkeypatch.setattr(torch, "empty", torch.zeros)
    N, W, H = 100, 32, 32
    sc, V = _scene(N, W, H)
    cfg = F.FusedCfg(width=W, height=H, sh_degree=-1, mode="RGB", eps2d=0.3, near_plane=0.01, far_plane=1e10,
                     radius_clip=0.0, antialiased=False, ty0=0, ty1=2, want_isect_ids=True)
    with torch.no_grad():
        render, alphas, means2d, _ = F.fused_absgrad_apply(sc["means"], sc["quats"], sc["scales"], sc["opacities"],
                                                           torch.rand(N, 3), V, sc["K"].contiguous(), cfg)
    assert not means2d.requires_grad and not hasattr(means2d, "absgrad")


@no_gpu
@pytest.mark.parametrize("C,bg", [(2, False), (3, True)])
def test_staged_absgrad_calls_once_per_camera(C, bg, monkeypatch):
    import gsplatloc_amd.ops as O

    calls = []

    def refused(status, what):
        calls.append(what)
        assert status in (0, -3), (what, status)

    monkeypatch.setattr(O, "check", refused)
    monkeypatch.setattr(O, "current_stream", lambda: None)
    N, W, H, D = 50, 32, 32, 4
    th, tw = 2, 2
    means2d = (torch.rand(C, N, 2) * 32).requires_grad_()
    conics = torch.rand(C, N, 3).requires_grad_()
    colors = torch.rand(C, N, D).requires_grad_()
    opac = torch.rand(C, N).requires_grad_()
    backgrounds = torch.rand(C, D) if bg else None
    offsets = torch.zeros(C, th, tw, dtype=torch.int32)  # every list ends at the last tile: 5 entries there
    flatten_ids = torch.arange(5, dtype=torch.int32)
    render, alphas = O._RasterizeToPixels.apply(means2d, conics, colors, opac, backgrounds, W, H, 16, offsets,
                                                flatten_ids, True)
    assert render.shape == (C, H, W, D) and alphas.shape == (C, H, W, 1)
    (render.sum() + alphas.sum()).backward()
    assert calls == (["gsl_rasterize_fwd"] * C + ["gsl_rasterize_bwd"] * C + ["gsl_vacc_unpack"] +
                     ["gsl_rasterize_absgrad"] * C)
    assert means2d.absgrad.shape == (C, N, 2)
    assert means2d.grad.shape == (C, N, 2)


def test_chunked_features_refuse_absgrad():
    """Features wider than a compositing chunk: |sum over chunks| is not the sum of per-chunk |.| -- refused before
    anything touches a device (host tensors here)."""
    from gsplatloc_amd import rasterization

    N, C = 20, 2
    kw = dict(means=torch.zeros(N, 3), quats=torch.zeros(N, 4), scales=torch.zeros(N, 3), opacities=torch.zeros(N),
              viewmats=torch.eye(4)[None].repeat(C, 1, 1), Ks=torch.eye(3)[None].repeat(C, 1, 1), width=32, height=32)
    with pytest.raises(NotImplementedError, match="chunks"):
        rasterization(colors=torch.zeros(N, 40), absgrad=True, **kw)
    with pytest.raises(NotImplementedError, match="chunks"):
        rasterization(colors=torch.zeros(N, 32), absgrad=True, render_mode="RGB+ED", **kw)
    with pytest.raises(NotImplementedError, match="chunks"):
        rasterization(colors=torch.zeros(N, 16), absgrad=True, channel_chunk=8, **kw)
