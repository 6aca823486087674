"""Packed projection and sparse gradients on the GPU (packed=True, sparse_grad=True).

The yardstick is the DENSE path of this repository plus the float64 oracle: tests/packed_ref.pack(dense) are the rows
of the dense [C,N,...] tensors at nonzero(radii > 0) in row-major order.  The packed kernels call the dense kernel's
device function (csrc/project_dev.h, project_pair), so floats are compared with torch.equal.

Gradients of a whole render are compared with bounds, not bit for bit, also where only the store address of the
projection backward differs (sparse against dense mode, one camera): the compositing backward in front of it sums
per-Gaussian gradients with float atomics, so two runs of the SAME path already differ in the last bits.  The
bit-for-bit statement is tested where its premise holds: the projection operator alone, fed the same upstream
gradients twice.
"""
import math

import pytest
import torch

from oracle import gsplat_oracle as G
from tests import packed_ref
from tests.grad_paths import compare_grads, failing_subsets
from tests.parity import IMAGE_ATOL, IMAGE_RTOL, POSE_GRAD_TOL, agreeing_pixels, rel_inf
from tests.scenes import frustum_clamp_scene, random_scene, sh_from_rgb, small_pose

pytestmark = pytest.mark.gpu

DEV = "cuda"
MODES = ["RGB", "D", "ED", "RGB+D", "RGB+ED"]
CASES = ["all_visible", "mostly_offscreen", "nothing_visible", "one_gaussian", "straddle", "clip_and_clamp",
         "antialiased"]


def _gpu():
    import gsplatloc_amd as A

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return A


def _poses(C, rot=3.0, trans=0.15):
    return torch.stack([torch.linalg.inv(small_pose(rot, trans, seed=11 + c, dtype=torch.float32)) for c in range(C)])


def _case(name, C):
    """Inputs (float32, on the device) of one case: dict(means, quats, scales, opacities, rgbs, Vs [C,4,4],
    Ks [C,3,3], W, H, kw (cull arguments), aa)."""
    W, H, kw, aa = 160, 120, {}, False
    if name == "clip_and_clamp":  # near / far / radius_clip / frustum clamp
        sc = frustum_clamp_scene(dtype=torch.float32)
        W, H, kw = sc["W"], sc["H"], sc["kw"]
        Vs = torch.stack([sc["V"]] + [torch.linalg.inv(small_pose(2.0 + c, 0.05, seed=4 + c, dtype=torch.float32))
                                      for c in range(1, C)])
    else:
        N = {"one_gaussian": 1, "straddle": 1999}.get(name, 2000)  # 1999, 2000: not multiples of 64
        sc = random_scene(N, W, H, seed=21, sigma_px=1.5, aniso=True, opacity=(0.3, 0.95), dtype=torch.float32)
        if name == "mostly_offscreen":
            sc["means"][:, :2] *= 5.0
        elif name == "nothing_visible":
            sc["means"][:, 2] *= -1.0
        elif name == "one_gaussian":
            sc["means"][0] = torch.tensor([0.05, -0.02, 2.0])
        Vs = _poses(C, rot=0.5, trans=0.01) if name == "one_gaussian" else _poses(C)
        aa = name == "antialiased"
    out = {k: sc[k].to(DEV) for k in ("means", "quats", "scales", "opacities", "rgbs")}
    # Ks is a stride-0 view on the device (expanded after the copy: copying an expanded tensor makes it dense): the staged
    # wrappers accept it, see test_stride_0_Ks_gives_the_contiguous_result
    out.update(Vs=Vs.to(DEV), Ks=sc["K"].to(DEV)[None].expand(C, 3, 3), W=W, H=H, kw=kw, aa=aa)
    return out


def _project(A, sc, packed, **more):
    return A.fully_fused_projection(sc["means"], None, sc["quats"], sc["scales"], sc["Vs"], sc["Ks"], sc["W"],
                                    sc["H"], packed=packed, calc_compensations=sc["aa"], **sc["kw"], **more)


def _check_case(name, nnz, total):
    if name == "nothing_visible":
        assert nnz == 0
    elif name == "all_visible":
        assert nnz > 0.9 * total
    elif name == "mostly_offscreen":
        assert 0 < nnz < 0.25 * total
    else:
        assert nnz > 0


# --------------------------------------------------------------------------- 5. projection forward
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("name", CASES)
def test_packed_projection_is_the_dense_projection_packed(name, C):
    A = _gpu()
    sc = _case(name, C)
    want = packed_ref.pack(_project(A, sc, packed=False))
    got = packed_ref.as_dict(_project(A, sc, packed=True))
    _check_case(name, got["camera_ids"].numel(), C * sc["means"].shape[0])
    assert got["camera_ids"].dtype == torch.int64 and got["gaussian_ids"].dtype == torch.int64
    assert got["radii"].dtype == torch.int32
    for k in ("camera_ids", "gaussian_ids", "radii"):
        assert torch.equal(got[k], want[k]), (k, got[k].shape, want[k].shape)
    for k in ("means2d", "depths", "conics", "compensations"):
        if want[k] is None:
            assert got[k] is None
            continue
        assert got[k].shape == want[k].shape, k
        same = got[k] == want[k]
        assert bool(same.all()), (k, int((~same).sum()), float((got[k] - want[k]).abs().max()))


@pytest.mark.parametrize("packed", [False, True])
def test_stride_0_Ks_gives_the_contiguous_result(packed, monkeypatch):
    """_case() hands every test of this file one K expanded to [C,3,3] with stride 0; the projection wrappers make it
    contiguous themselves.  Same bits as with a contiguous copy, from the operator and from rasterization()."""
    A = _gpu()
    sc = _case("antialiased", 3)
    assert sc["Ks"].stride(0) == 0 and not sc["Ks"].is_contiguous()
    dense = dict(sc, Ks=sc["Ks"].contiguous())
    for a, b in zip(_project(A, sc, packed=packed), _project(A, dense, packed=packed)):
        assert torch.equal(a, b)
    via = "sparse" if packed else "dense"
    r0, a0, _, _ = _render(A, sc, "RGB+ED", monkeypatch, via, sh=1)
    r1, a1, _, _ = _render(A, dense, "RGB+ED", monkeypatch, via, sh=1)
    assert torch.equal(r0, r1) and torch.equal(a0, a1)


def test_packed_projection_across_many_workgroups():
    """70 001 Gaussians, 4 cameras (1 094 workgroups, a scan chunk of 5 per thread), a tenth of the pairs visible."""
    A = _gpu()
    sc = _case("all_visible", 4)
    big = random_scene(70001, 160, 120, seed=3, sigma_px=1.0, aniso=True, dtype=torch.float32)
    big["means"][:, :2] *= 3.0
    sc.update({k: big[k].to(DEV) for k in ("means", "quats", "scales", "opacities", "rgbs")})
    want = packed_ref.pack(_project(A, sc, packed=False))
    got = packed_ref.as_dict(_project(A, sc, packed=True))
    assert 0 < got["camera_ids"].numel() < 0.2 * 4 * 70001
    for k in packed_ref.NAMES[:6]:
        assert torch.equal(got[k], want[k]), k


# --------------------------------------------------------------------------- 6. binning
@pytest.mark.parametrize("sort", [True, False])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("name", CASES)
def test_packed_isect_tiles_equals_dense(name, C, sort):
    A = _gpu()
    sc = _case(name, C)
    N = sc["means"].shape[0]
    tw, th = -(-sc["W"] // 16), -(-sc["H"] // 16)
    radii, means2d, depths, _, _ = _project(A, sc, packed=False)
    tpg_d, ids_d, flat_d = A.isect_tiles(means2d, radii, depths, 16, tw, th, sort=sort)
    p = packed_ref.as_dict(_project(A, sc, packed=True))
    tpg_p, ids_p, flat_p = A.isect_tiles(p["means2d"], p["radii"], p["depths"], 16, tw, th, sort=sort, packed=True,
                                         n_cameras=C, camera_ids=p["camera_ids"], gaussian_ids=p["gaussian_ids"])
    assert tpg_p.shape == p["radii"].shape and tpg_p.dtype == torch.int32
    assert torch.equal(tpg_p, packed_ref.pack_rows(tpg_d, radii))
    assert torch.equal(ids_p, ids_d)
    assert flat_p.dtype == torch.int32 and flat_p.shape == flat_d.shape
    back = p["camera_ids"][flat_p.long()] * N + p["gaussian_ids"][flat_p.long()]
    assert torch.equal(back, flat_d.long())
    if sort:  # (offsets are defined for sorted keys only)
        assert torch.equal(A.isect_offset_encode(ids_p, C, tw, th), A.isect_offset_encode(ids_d, C, tw, th))


# --------------------------------------------------------------------------- 7. render
def _render(A, sc, mode, monkeypatch, via, sh=None, bg=None, colors=None, grad=False, **more):
    """rasterization() through the staged dense path ("dense"), the packed pipeline with dense gradients ("env":
    GSLOC_PACKED=1) or with sparse ones ("sparse").  Returns (render, alphas, meta, inputs with .grad)."""
    monkeypatch.setenv("GSLOC_DISABLE_FUSED", "1")
    monkeypatch.setenv("GSLOC_PACKED", "1" if via == "env" else "0")
    if colors is None:
        colors = sc["rgbs"] if sh is None else sh_from_rgb(sc["rgbs"].cpu()).to(DEV)
    ins = dict(means=sc["means"], quats=sc["quats"], scales=sc["scales"], opacities=sc["opacities"], colors=colors,
               viewmats=sc["Vs"])
    ins = {k: v.detach().clone().requires_grad_(grad) for k, v in ins.items()}
    r, a, meta = A.rasterization(**ins, Ks=sc["Ks"], width=sc["W"], height=sc["H"], sh_degree=sh, render_mode=mode,
                                 backgrounds=bg, packed=True, sparse_grad=(via == "sparse"),
                                 rasterize_mode="antialiased" if sc["aa"] else "classic", **sc["kw"], **more)
    return r, a, meta, ins


def _check_packed_meta(meta, dense_meta, C, N):
    nnz = meta["camera_ids"].numel()
    assert meta["camera_ids"].dtype == torch.int64 and meta["gaussian_ids"].shape == (nnz,)
    radii = dense_meta["radii"]
    assert torch.equal(meta["camera_ids"] * N + meta["gaussian_ids"], torch.nonzero(radii.reshape(-1) > 0)[:, 0])
    for k in ("radii", "means2d", "depths", "conics", "opacities", "tiles_per_gauss"):
        assert meta[k].shape[0] == nnz, k
        assert torch.equal(meta[k], packed_ref.pack_rows(dense_meta[k], radii)), k
    assert meta["n_cameras"] == C and torch.equal(meta["isect_offsets"], dense_meta["isect_offsets"])
    assert torch.equal(meta["isect_ids"], dense_meta["isect_ids"])


@pytest.mark.parametrize("with_bg", [False, True])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("mode", MODES)
def test_packed_render_is_bit_identical_to_the_staged_dense_render(mode, C, with_bg, monkeypatch):
    A = _gpu()
    sc = _case("mostly_offscreen" if C == 3 else "all_visible", C)
    sh = 1 if mode in ("RGB+ED", "RGB+D") else None
    n_rgb = 3 if mode.startswith("RGB") else 0
    bg = torch.rand(C, n_rgb, generator=torch.Generator().manual_seed(5)).to(DEV) if with_bg else None
    r_d, a_d, m_d, _ = _render(A, sc, mode, monkeypatch, "dense", sh=sh, bg=bg)
    assert m_d["camera_ids"] is None and m_d["radii"].shape == (C, sc["means"].shape[0])  # the default stays dense
    for via in ("sparse", "env"):
        r_p, a_p, m_p, _ = _render(A, sc, mode, monkeypatch, via, sh=sh, bg=bg)
        assert torch.equal(r_p, r_d), (via, float((r_p - r_d).abs().max()))
        assert torch.equal(a_p, a_d), via
        _check_packed_meta(m_p, m_d, C, sc["means"].shape[0])


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("name", CASES)
def test_packed_render_cases_forward_and_backward(name, C, monkeypatch):
    """Every case (nothing visible included: nnz == 0 end to end, backward too) renders the staged dense path's image
    and yields finite gradients of the right shapes."""
    A = _gpu()
    sc = _case(name, C)
    N = sc["means"].shape[0]
    r_d, a_d, m_d, _ = _render(A, sc, "RGB+ED", monkeypatch, "dense", sh=1)
    for via in ("sparse", "env"):
        r_p, a_p, m_p, ins = _render(A, sc, "RGB+ED", monkeypatch, via, sh=1, grad=True)
        assert torch.equal(r_p, r_d) and torch.equal(a_p, a_d), via
        _check_packed_meta(m_p, m_d, C, N)
        _check_case(name, m_p["camera_ids"].numel(), C * N)
        (r_p.sum() + a_p.sum()).backward()
        for k, t in ins.items():
            g = t.grad.to_dense() if t.grad.is_sparse else t.grad
            assert g.shape == t.shape and bool(torch.isfinite(g).all()), (via, k)
            if name == "nothing_visible":
                assert not bool(g.any()), (via, k)


def test_packed_render_33_channels_in_chunks(monkeypatch):
    A = _gpu()
    sc = _case("mostly_offscreen", 3)
    g = torch.Generator().manual_seed(12)
    feats, bg = torch.rand(sc["means"].shape[0], 32, generator=g).to(DEV), torch.rand(3, 32, generator=g).to(DEV)
    for chunk in (32, 7):
        r_d, a_d, _, _ = _render(A, sc, "RGB+ED", monkeypatch, "dense", colors=feats, bg=bg, channel_chunk=chunk)
        assert r_d.shape == (3, sc["H"], sc["W"], 33)
        for via in ("sparse", "env"):
            r_p, a_p, _, _ = _render(A, sc, "RGB+ED", monkeypatch, via, colors=feats, bg=bg, channel_chunk=chunk)
            assert torch.equal(r_p, r_d) and torch.equal(a_p, a_d), (via, chunk)


def test_packed_render_per_camera_colours(monkeypatch):
    """colors [C,N,D] and SH coefficients [C,N,K,3]: gathered by (camera_ids, gaussian_ids)."""
    A = _gpu()
    sc = _case("mostly_offscreen", 3)
    N = sc["means"].shape[0]
    g = torch.Generator().manual_seed(13)
    for sh, colors in ((None, torch.rand(3, N, 3, generator=g)), (1, torch.randn(3, N, 4, 3, generator=g) * 0.3)):
        r_d, a_d, _, _ = _render(A, sc, "RGB", monkeypatch, "dense", sh=sh, colors=colors.to(DEV))
        r_p, a_p, _, _ = _render(A, sc, "RGB", monkeypatch, "sparse", sh=sh, colors=colors.to(DEV))
        assert torch.equal(r_p, r_d) and torch.equal(a_p, a_d), sh


@pytest.mark.parametrize("mode,sh", [("RGB+ED", 1), ("RGB", None), ("ED", 1)])
def test_packed_render_against_the_float64_oracle(mode, sh, monkeypatch):
    """The bounds the staged dense path is held to in test_gpu_parity.py::test_rasterization_end_to_end (render and
    alpha within 1e-4 relative + 2e-5 but for 3e-3 of the elements, pose gradient within POSE_GRAD_TOL on the pixels
    both sides agree on), three cameras."""
    A = _gpu()
    C = 3
    sc = _case("mostly_offscreen", C)
    colors = sc["rgbs"] if sh is None else sh_from_rgb(sc["rgbs"].cpu()).to(DEV)
    Vo = sc["Vs"].cpu().double().clone().requires_grad_()
    r_o, a_o, _ = G.rasterization(sc["means"].cpu().double(), sc["quats"].cpu().double(), sc["scales"].cpu().double(),
                                  sc["opacities"].cpu().double(), colors.cpu().double(), Vo, sc["Ks"].cpu().double(),
                                  sc["W"], sc["H"], sh_degree=sh, render_mode=mode)
    r_p, a_p, _, ins = _render(A, sc, mode, monkeypatch, "sparse", sh=sh, grad=True)
    for got, want, what in ((r_p, r_o, "render"), (a_p, a_o, "alpha")):
        d = (got.detach().cpu().double() - want.detach()).abs()
        frac = (d > 2e-5 + 1e-4 * want.detach().abs()).double().mean().item()
        print(f"[packed] {mode} {what}: {frac:.2e} of the elements outside")
        assert frac <= 3e-3, (what, frac)
    ok = agreeing_pixels(r_p, a_p, r_o, a_o)
    v = torch.randn(r_o.shape, generator=torch.Generator().manual_seed(2)) * ok[..., None]
    (r_o * v.double()).sum().backward()
    (r_p * v.to(DEV)).sum().backward()
    err = rel_inf(ins["viewmats"].grad[:, :3], Vo.grad[:, :3])
    print(f"[packed] {mode} v_viewmats against float64: {err:.2e}")
    assert not ins["viewmats"].grad.is_sparse
    assert err < POSE_GRAD_TOL, err


def test_gsmodel_with_packed_sparse_config_renders_the_default_configs_image():
    """GSModel(config=GsConfig(packed=True, sparse_grad=True)) against the default config (which takes the fused
    one-camera path: another kernel, so the images agree within parity.IMAGE_RTOL / IMAGE_ATOL, but for the bounded
    fraction of threshold pixels test_gpu_parity.py allows)."""
    _gpu()
    from gsplatloc_amd.my_gsplat.model import GSModel, GsConfig

    sc = _case("all_visible", 1)
    c2w = torch.linalg.inv(sc["Vs"])
    out = {}
    for name, cfg in (("default", GsConfig()), ("packed", GsConfig(packed=True, sparse_grad=True))):
        model = GSModel(sc["means"], sc["rgbs"], config=cfg, scales=sc["scales"])
        out[name] = model(c2w, sc["Ks"], sc["W"], sc["H"])
    assert out["default"][2]["camera_ids"] is None
    assert out["packed"][2]["camera_ids"].numel() == int((out["default"][2]["radii"] > 0).sum())
    ok = agreeing_pixels(out["packed"][0], out["packed"][1], out["default"][0], out["default"][1],
                         rtol=IMAGE_RTOL, atol=IMAGE_ATOL)
    flipped = 1.0 - ok.double().mean().item()
    print(f"[packed] GSModel packed/sparse against default: flipped pixels {flipped:.2e}")
    assert flipped <= 3e-3, flipped


# --------------------------------------------------------------------------- 8. / 9. gradients
GRAD_NAMES = ("means", "quats", "scales", "colors", "opacities")


def _grads(A, sc, via, monkeypatch, v, va, sh, mode="RGB+ED"):
    r, a, meta, ins = _render(A, sc, mode, monkeypatch, via, sh=sh, grad=True)
    ((r * v).sum() + (a * va).sum()).backward()
    torch.cuda.synchronize()
    return ins, meta


@pytest.mark.parametrize("name,C,sh", [("all_visible", 1, 1), ("mostly_offscreen", 3, 1), ("antialiased", 3, None),
                                       ("straddle", 3, 1), ("clip_and_clamp", 1, None)])
def test_packed_gradients_dense_mode(name, C, sh, monkeypatch):
    """GSLOC_PACKED=1 against the staged dense path: per-Gaussian gradients with grad_paths.compare_grads and its
    constants as they are, v_viewmats within parity.POSE_GRAD_TOL (float32 sums of the same terms in another order)."""
    A = _gpu()
    sc = _case(name, C)
    N = sc["means"].shape[0]
    g = torch.Generator().manual_seed(8)
    v = torch.randn(C, sc["H"], sc["W"], 4, generator=g).to(DEV)
    va = torch.randn(C, sc["H"], sc["W"], 1, generator=g).to(DEV)
    want, m_d = _grads(A, sc, "dense", monkeypatch, v, va, sh)
    got, m_p = _grads(A, sc, "env", monkeypatch, v, va, sh)
    seen = torch.unique(m_p["gaussian_ids"]).cpu()
    assert seen.numel() > 0
    for k in GRAD_NAMES:
        assert not got[k].grad.is_sparse and got[k].grad.shape == want[k].grad.shape, k
    worst, counts, _ = compare_grads({k: got[k].grad for k in GRAD_NAMES}, {k: want[k].grad for k in GRAD_NAMES},
                                     {"all": torch.arange(N), "visible": seen})
    err = rel_inf(got["viewmats"].grad, want["viewmats"].grad)
    print(f"[packed] dense-mode gradients {name} C={C}: worst {worst}, outliers {counts}, v_viewmats {err:.2e}")
    assert not failing_subsets(counts), (counts, worst)
    assert err < POSE_GRAD_TOL, err
    hidden = torch.ones(N, dtype=torch.bool)
    hidden[seen] = False
    for k in ("means", "quats", "scales"):  # a Gaussian no camera sees gets exactly zero
        assert not bool(got[k].grad.cpu()[hidden].any()), k


@pytest.mark.parametrize("C", [1, 3])
def test_packed_gradients_sparse_mode(C, monkeypatch):
    """sparse_grad=True: sparse COO gradients over gaussian_ids (coalesced iff one camera), dense v_viewmats, values
    within the bounds of the dense-mode test of the dense-mode gradients (module docstring: why not bit for bit
    here), and one SparseAdam step that moves visible rows only."""
    A = _gpu()
    sc = _case("mostly_offscreen", C)
    N = sc["means"].shape[0]
    g = torch.Generator().manual_seed(9)
    v = torch.randn(C, sc["H"], sc["W"], 4, generator=g).to(DEV)
    va = torch.randn(C, sc["H"], sc["W"], 1, generator=g).to(DEV)
    want, _ = _grads(A, sc, "env", monkeypatch, v, va, None)
    got, meta = _grads(A, sc, "sparse", monkeypatch, v, va, None)
    gids = meta["gaussian_ids"]
    for k in ("means", "quats", "scales"):
        gr = got[k].grad
        assert gr.is_sparse and gr.shape == got[k].shape, k
        assert gr.is_coalesced() == (C == 1), k
        assert torch.equal(gr._indices(), gids[None]) and gr._values().shape == (gids.numel(),) + got[k].shape[1:], k
    assert not got["viewmats"].grad.is_sparse and got["viewmats"].grad.shape == (C, 4, 4)
    dense = {k: (got[k].grad.to_dense() if got[k].grad.is_sparse else got[k].grad) for k in GRAD_NAMES}
    seen = torch.unique(gids).cpu()
    worst, counts, _ = compare_grads(dense, {k: want[k].grad for k in GRAD_NAMES},
                                     {"all": torch.arange(N), "visible": seen})
    err = rel_inf(got["viewmats"].grad, want["viewmats"].grad)
    print(f"[packed] sparse-mode gradients C={C}: worst {worst}, outliers {counts}, v_viewmats {err:.2e}")
    assert not failing_subsets(counts), (counts, worst)
    assert err < POSE_GRAD_TOL, err
    # one optimiser step on the sparse gradient
    means = got["means"]
    before = means.detach().clone()
    torch.optim.SparseAdam([means], lr=1e-2).step()
    moved = (means.detach() != before).any(1).cpu()
    has_grad = (dense["means"] != 0).any(1).cpu()
    hidden = torch.ones(N, dtype=torch.bool)
    hidden[seen] = False
    assert not bool(moved[hidden].any()) and not bool(moved[~has_grad].any())
    sizeable = (dense["means"].abs() > 1e-3 * dense["means"].abs().max()).any(1).cpu()  # Adam's step is ~ lr there
    assert bool(sizeable.any()) and bool(moved[sizeable].all())


@pytest.mark.parametrize("C", [1, 3])
def test_packed_projection_backward_sparse_and_dense_store_the_same_values(C):
    """The projection operator alone, the same upstream gradients twice: sparse values scattered to [N,.] equal the
    dense-mode gradient bit for bit for one camera (same kernel, same values, only the store address differs); for
    three cameras the dense mode sums a Gaussian's rows with float atomics, the sparse tensor keeps them apart:
    within GRAD_RTOL / GRAD_ATOL.  v_viewmats is a fixed-order sum: bit for bit where both modes run the same kernel
    instance (one camera).  Against the dense operator's backward: same bounds."""
    A = _gpu()
    sc = _case("antialiased", C)
    N = sc["means"].shape[0]
    out = {}
    for mode in ("dense_op", "packed", "sparse"):
        ins = {k: sc[k].detach().clone().requires_grad_() for k in ("means", "quats", "scales", "Vs")}
        res = A.fully_fused_projection(ins["means"], None, ins["quats"], ins["scales"], ins["Vs"], sc["Ks"], sc["W"],
                                       sc["H"], packed=(mode != "dense_op"), sparse_grad=(mode == "sparse"),
                                       calc_compensations=True)
        if mode == "dense_op":
            radii = res[0]
            g = torch.Generator().manual_seed(3)
            ups = [torch.randn(t.shape, generator=g).to(DEV) for t in res[1:]]
            loss = sum((t * u).sum() for t, u in zip(res[1:], ups))
        else:
            loss = sum((t * packed_ref.pack_rows(u, radii)).sum() for t, u in zip(res[3:], ups))
        loss.backward()
        out[mode] = {k: t.grad for k, t in ins.items()}
    for k in ("means", "quats", "scales"):
        sp = out["sparse"][k]
        assert sp.is_sparse and sp.is_coalesced() == (C == 1)
        if C == 1:
            assert torch.equal(sp.to_dense(), out["packed"][k]), k
    if C == 1:  # the same kernel instance
        assert torch.equal(out["sparse"]["Vs"], out["packed"]["Vs"])
    names = ("means", "quats", "scales")
    subsets = {"all": torch.arange(N)}
    for a, b in (("sparse", "packed"), ("packed", "dense_op")):
        got = {k: (out[a][k].to_dense() if out[a][k].is_sparse else out[a][k]) for k in names}
        worst, counts, _ = compare_grads(got, {k: out[b][k] for k in names}, subsets)
        err = rel_inf(out[a]["Vs"], out[b]["Vs"])
        print(f"[packed] projection backward {a} against {b}, C={C}: worst {worst}, v_viewmats {err:.2e}")
        assert not failing_subsets(counts), (a, b, counts, worst)
        assert err < POSE_GRAD_TOL, (a, b, err)


def test_packed_projection_pose_only_backward():
    """Only viewmats requires a gradient: no Gaussian gradients are allocated, v_viewmats equals the full call's."""
    A = _gpu()
    sc = _case("mostly_offscreen", 3)
    grads = []
    for full in (True, False):
        ins = {k: sc[k].detach().clone().requires_grad_(full or k == "Vs") for k in ("means", "quats", "scales", "Vs")}
        res = A.fully_fused_projection(ins["means"], None, ins["quats"], ins["scales"], ins["Vs"], sc["Ks"], sc["W"],
                                       sc["H"], packed=True)
        (res[3].sum() + (res[4] * res[4]).sum() + res[5].sum()).backward()
        assert (ins["means"].grad is not None) == full
        grads.append(ins["Vs"].grad)
    # two template instantiations of one kernel: the compiler may contract FMAs differently
    assert rel_inf(grads[1], grads[0]) < 1e-6


@pytest.mark.parametrize("shape,n_ids,unique", [((500, 3), 300, True), ((500,), 2000, False), ((3, 3), 5000, False),
                                                 ((700, 4, 3), 1999, False), ((64,), 0, False)])
def test_gather_rows_and_its_backward(shape, n_ids, unique):
    """ops.gather_rows (what the packed pipeline reads per-Gaussian and per-camera tensors with) against torch's
    indexing: forward exact; backward exact where no id repeats; where float atomics add, within 2e-4 of the largest
    entry (at most ~1 700 terms per row here, float32 worst case n * 2^-24 = 1e-4 on either side's sum; sorted ids with long
    runs of one value included: the per-camera case)."""
    _gpu()
    from gsplatloc_amd.ops import gather_rows

    g = torch.Generator().manual_seed(4)
    n = shape[0]
    ids = torch.randperm(n, generator=g)[:n_ids] if unique else torch.sort(torch.randint(0, n, (n_ids,), generator=g))[0]
    ids = ids.to(DEV)
    a = torch.randn(shape, generator=g).to(DEV).requires_grad_()
    b = a.detach().clone().requires_grad_()
    ra, rb = gather_rows(a, ids, unique=unique), b[ids]
    assert torch.equal(ra, rb)
    up = torch.randn(rb.shape, generator=g).to(DEV)
    (ra * up).sum().backward()
    (rb * up).sum().backward()
    if unique:
        assert torch.equal(a.grad, b.grad)
    elif n_ids:
        assert rel_inf(a.grad, b.grad) < 2e-4
    else:
        assert not bool(a.grad.any())


# --------------------------------------------------------------------------- 10. absgrad
def _agree(ours, ref, what, tol=1e-4, frac=0.002):
    """The rule of tests/test_gpu_absgrad.py with its defaults: per Gaussian, within tol of the largest reference
    value; ceil(frac) outliers for pixels on a threshold."""
    ours, ref = ours.detach().double().cpu(), ref.detach().double().cpu()
    assert torch.isfinite(ours).all(), what
    scale = float(ref.abs().max())
    assert scale > 0, what
    bad = ((ours - ref).abs().amax(-1) > tol * scale)
    n_bad = int(bad.sum())
    assert n_bad <= math.ceil(frac * bad.numel()), (what, n_bad, float((ours - ref).abs().max()) / scale)


@pytest.mark.parametrize("via", ["sparse", "env"])
@pytest.mark.parametrize("C", [1, 3])
def test_packed_absgrad(C, via, monkeypatch):
    A = _gpu()
    sc = _case("mostly_offscreen" if C == 3 else "all_visible", C)
    g = torch.Generator().manual_seed(10)
    v = torch.randn(C, sc["H"], sc["W"], 4, generator=g).to(DEV)
    res = {}
    for how in ("dense", via):
        r, a, meta, _ = _render(A, sc, "RGB+ED", monkeypatch, how, sh=1, grad=True, absgrad=True)
        meta["means2d"].retain_grad()
        ((r * v).sum() + a.sum()).backward()
        res[how] = meta
    radii = res["dense"]["radii"]
    nnz = int((radii > 0).sum())
    ab = res[via]["means2d"].absgrad
    assert ab.shape == (nnz, 2) and res[via]["means2d"].grad.shape == (nnz, 2)
    _agree(ab, packed_ref.pack_rows(res["dense"]["means2d"].absgrad, radii), f"absgrad C={C} {via}")
    _agree(res[via]["means2d"].grad, packed_ref.pack_rows(res["dense"]["means2d"].grad, radii), f"grad C={C} {via}")


# --------------------------------------------------------------------------- 11. memory
def sparse_view_scene(N, C=4, W=160, H=120, seed=17):
    """C cameras over a cloud five times as wide as a frustum in x and y: at most a tenth of the pairs visible."""
    sc = _case("all_visible", C)
    big = random_scene(N, W, H, seed=seed, sigma_px=1.0, aniso=True, opacity=(0.3, 0.95), dtype=torch.float32)
    big["means"][:, :2] *= 5.0
    sc.update({k: big[k].to(DEV) for k in ("means", "quats", "scales", "opacities", "rgbs")})
    return sc


def test_packed_pipeline_peaks_below_the_dense_one_when_little_is_visible(monkeypatch):
    """C = 4, at most 10 % of the pairs visible: the dense path's intermediates are [C,N,...] (32 B of projection
    outputs, 16 B of features and a 64-B gradient row per pair), the packed pipeline's [nnz,...] plus 40 B of ballots
    and offsets per 256 pairs -- so its peak must be strictly lower.  A condition of the layouts; the measured ratio
    is in DESIGN.md."""
    A = _gpu()
    C, N = 4, 200_000
    sc = sparse_view_scene(N, C)
    v = torch.randn(C, sc["H"], sc["W"], 4, generator=torch.Generator().manual_seed(1)).to(DEV)
    peak = {}
    for via in ("dense", "env", "sparse"):
        for it in range(2):  # a warm-up call, then the measured one
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            r, a, meta, ins = _render(A, sc, "RGB+ED", monkeypatch, via, grad=True)
            ((r * v).sum() + a.sum()).backward()
            torch.cuda.synchronize()
            peak[via] = torch.cuda.max_memory_allocated() - base
            if via != "dense":
                share = meta["camera_ids"].numel() / (C * N)
                assert 0 < share <= 0.10, share
            del r, a, meta, ins
    print(f"[packed] peak bytes above the inputs, C={C} N={N}: {peak}; packed / dense = "
          f"{peak['env'] / peak['dense']:.3f} (dense gradients), {peak['sparse'] / peak['dense']:.3f} (sparse)")
    assert peak["env"] < peak["dense"] and peak["sparse"] < peak["dense"], peak
