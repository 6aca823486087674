"""Every projection path at cameras with fx != fy, an off-centre fractional principal point and a different K per camera
(tests/cameras.py), element by element against the float64 oracle on the same float32 inputs.

The stage operators (dense and packed projection, rasterization() on the staged route) run on three_cameras: Ks =
(wide_x, wide_y, control) and three poses; everything is compared PER CAMERA, so a kernel or wrapper that reads camera
0's K for every camera, or puts a pose gradient into a neighbour's slot, fails.  The fused one-camera path runs at wide_x
and wide_y through RenderContext and through the drop-in rasterization() call.

tests/test_cameras_cpu.py shows on these very inputs that each wrong camera (fx <-> fy, cx <-> cy, a centred principal
point, camera 0's K everywhere) lands at least 100 x outside these bounds and that the float32 oracle stays inside
them.  Bounds and figures: tests/camera_checks.py (a figure is measured / bound; 1.0 is the bound).
"""
import functools

import pytest
import torch

from tests import camera_checks as X
from tests import cameras as cam
from tests import packed_ref
from tests.grad_paths import failing_subsets
from tests.parity import POSE_GRAD_TOL, rel_inf, report
from tests.test_gpu_parity import mostly_close

pytestmark = pytest.mark.gpu

DEV = "cuda"
GAUSS = ("means", "quats", "scales")
POSE_ONLY_TOL = 1e-6  # pose-only against full backward, as test_projection_pose_only_matches_full bounds it


def _gpu():
    import gsplatloc_amd as A
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return A


def _dense(t):
    return X.f64(t.coalesce().to_dense() if t.is_sparse else t)


def _report(tag, flipped, figs, counts):
    report(tag, max(flipped) if flipped else 0.0, **{k: v for k, v in figs.items()},
           **{"outliers " + k: float(c[0]) for k, c in counts.items()})


# ---- the stage operators: projection ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _projection_oracle():
    return X.oracle_projection(cam.projection_case())


class _HipProjection:
    """A.fully_fused_projection on projection_case(); packed results are scattered back to [C,N,...] (by torch, so the
    upstream gradients reach the packed rows)."""

    def __init__(self, A, sc, packed=False, sparse_grad=False):
        self.ins = {k: sc[k].to(DEV).clone().requires_grad_() for k in GAUSS}
        self.ins["viewmats"] = sc["Vs"].to(DEV).clone().requires_grad_()
        res = A.fully_fused_projection(self.ins["means"], None, self.ins["quats"], self.ins["scales"], self.ins["viewmats"],
                                       sc["Ks"].to(DEV), sc["W"], sc["H"], packed=packed, sparse_grad=sparse_grad,
                                       calc_compensations=True, **sc["kw"])
        self.raw = res
        if packed:
            C, N = sc["Vs"].shape[0], sc["N"]
            ci, gi = res[0], res[1]
            full = lambda t: t.new_zeros((C, N) + tuple(t.shape[1:])).index_put((ci, gi), t)  # noqa: E731
            self.radii, self.outputs = full(res[2]), tuple(full(t) for t in res[3:])
        else:
            self.radii, self.outputs = res[0], tuple(res[1:])

    def grads(self, *upstream):
        sum((o * u.float().to(DEV)).sum() for o, u in zip(self.outputs, upstream)).backward()
        torch.cuda.synchronize()
        self.raw_grads = {k: t.grad for k, t in self.ins.items()}
        return {k: _dense(t.grad) for k, t in self.ins.items()}


def _check_projection(tag, sc, got):
    want = _projection_oracle()
    figs, keep, counts, worst, g, g_o = X.projection_figures(sc, want, got)
    C = keep.shape[0]
    _report(tag, [], figs, counts)
    r_g = got.radii.cpu()
    assert int(keep.sum()) > 1000
    for c in range(C):
        assert (r_g[c] == want.radii[c]).float().mean() > X.RADII_AGREE, (tag, "radii of camera", c, figs[f"radii [{c}]"])
        for nm, a, b in zip(X.PROJ_OUT, got.outputs, want.outputs):
            mostly_close(a[c].detach().cpu()[keep[c]], b[c][keep[c]], what=f"{tag}: {nm} of camera {c}")
            rows = a[c].detach().cpu()[r_g[c] == 0]
            assert float(rows.abs().max()) == 0.0, (tag, "culled rows are not zero", nm, c)
        for name, rows in sc["culled"].items():
            assert int(r_g[c, rows].abs().max()) == 0, (tag, name, "not culled in camera", c)
    gv = g["viewmats"]
    for c in range(C):
        # each camera on its own: a sum over the cameras would hide a swapped slot; the neighbour's is rejected
        assert figs[f"v_viewmats [{c}]"] < 1.0, (tag, "v_viewmats of camera", c, figs[f"v_viewmats [{c}]"] * POSE_GRAD_TOL)
        assert float(gv[c, 3].abs().max()) == 0.0, (tag, "row 3 of v_viewmats", c)
        assert rel_inf(gv[(c + 1) % C, :3], g_o["viewmats"][c, :3]) >= POSE_GRAD_TOL, (tag, "a neighbour's slot passes", c)
    assert not failing_subsets(counts), (tag, "outlier Gaussians (count, size, allowed)", counts, worst)
    return figs


def test_dense_projection_per_camera_K():
    A = _gpu()
    sc = cam.projection_case()
    got = _HipProjection(A, sc)
    assert got.radii.shape == (3, sc["N"]) and got.outputs[3] is not None
    _check_projection("cameras: dense projection", sc, got)


@pytest.mark.parametrize("sparse_grad", [False, True], ids=["dense-grad", "sparse-grad"])
def test_packed_projection_per_camera_K(sparse_grad):
    A = _gpu()
    sc = cam.projection_case()
    N = sc["N"]
    dense = _HipProjection(A, sc)
    got = _HipProjection(A, sc, packed=True, sparse_grad=sparse_grad)
    p = packed_ref.as_dict(got.raw)
    want = packed_ref.pack(tuple(t.detach() for t in dense.raw))
    seen = (dense.radii > 0).sum(1).tolist()
    assert len(set(seen)) == 3, seen  # another visible set per camera
    assert torch.equal(p["camera_ids"] * N + p["gaussian_ids"], torch.nonzero(dense.radii.reshape(-1) > 0)[:, 0])
    for k in packed_ref.NAMES:  # the bits of the dense call's rows
        assert torch.equal(p[k].detach(), want[k]), k
    _check_projection(f"cameras: packed projection sparse_grad={sparse_grad}", sc, got)
    for k in GAUSS:
        assert got.raw_grads[k].is_sparse == sparse_grad, k
    assert not got.raw_grads["viewmats"].is_sparse


# ---- the stage operators: rasterization() on the staged route ------------------------------------------------------------
_STAGED = {}


def _staged_oracle(name):
    if name not in _STAGED:
        _STAGED.clear()
        ins, Ks, kw, sc = cam.staged_case(name)
        _STAGED[name] = X.oracle_staged(ins, Ks, kw)
    return _STAGED[name]


class _HipStaged:
    def __init__(self, A, ins, Ks, kw, packed):
        self.ins = {k: t.to(DEV).clone().requires_grad_() for k, t in ins.items() if t is not None}
        i = self.ins
        r, a, self.meta = A.rasterization(i["means"], i["quats"], i["scales"], i["opacities"], i["colors"], i["viewmats"],
                                          Ks.to(DEV), backgrounds=i.get("backgrounds"), packed=packed, **kw)
        self.outputs = (r, a)

    def grads(self, v, va):
        r, a = self.outputs
        ((r * v.float().to(DEV)).sum() + (a * va.float().to(DEV)).sum()).backward()
        torch.cuda.synchronize()
        return {k: (_dense(t.grad) if t.grad is not None else torch.zeros(t.shape, dtype=torch.float64))
                for k, t in self.ins.items()}


@pytest.mark.parametrize("name", list(cam.STAGED_CASES))
def test_staged_rasterization_per_camera_K(name, monkeypatch):
    A = _gpu()
    case = cam.STAGED_CASES[name]
    monkeypatch.setenv("GSLOC_PACKED", "1" if case["packed"] else "0")
    ins, Ks, kw, sc = cam.staged_case(name)
    want = _staged_oracle(name)
    got = _HipStaged(A, ins, Ks, kw, case["packed"])
    C, n = 3, sc["N"]
    assert got.outputs[0].shape == want.outputs[0].shape and got.outputs[1].shape == want.outputs[1].shape
    assert (got.meta["camera_ids"] is None) != case["packed"]  # the route ran (three cameras: never the fused one)
    if not case["packed"]:
        assert got.meta["means2d"].shape == (C, n, 2) and got.meta["isect_ids"] is not None
    figs, flipped, counts, worst, g, g_o = X.render_figures(want, got, X.staged_subsets(sc, want.radii))
    tag = f"cameras: staged {name}"
    _report(tag, flipped, figs, counts)
    for c in range(C):
        assert flipped[c] <= X.PIXEL_OUTLIERS, f"{tag}: {flipped[c]:.2e} of camera {c}'s pixels differ from the oracle"
        assert figs[f"v_viewmats [{c}]"] < 1.0, (tag, "v_viewmats of camera", c, figs[f"v_viewmats [{c}]"] * POSE_GRAD_TOL)
        assert rel_inf(g["viewmats"][(c + 1) % C, :3], g_o["viewmats"][c, :3]) >= POSE_GRAD_TOL, (tag, "a neighbour's slot passes", c)
    assert not failing_subsets(counts), (tag, "outlier Gaussians (count, size, allowed)", counts, worst)
    if case["bg"]:
        assert figs["v_backgrounds"] < 1.0, (tag, "v_backgrounds", figs["v_backgrounds"] * POSE_GRAD_TOL)
    if not case["mode"].startswith("RGB"):  # no colours used
        assert float(g["colors"].abs().max()) == 0.0, (tag, "a colour gradient in a depth-only mode")
    for name_, rows in sc["culled"].items():
        for k in ("means", "quats", "scales", "opacities"):
            assert float(g[k][rows].abs().max()) == 0.0, (tag, "a culled row with a gradient", name_, k)


# ---- the fused one-camera path ------------------------------------------------------------------------------------------
class _HipFused:
    def __init__(self, sc, case, full_grads=True, **more):
        from gsplatloc_amd.context import RenderContext
        rgb = case["mode"].startswith("RGB")
        self.rc = rc = RenderContext(sc["N"], sc["W"], sc["H"], case["mode"], sh_degree=1 if rgb else None, K_sh=4, device=DEV,
                                     full_grads=full_grads, **sc["planes"], **case["ctx"], **more)
        self.args = [sc[k].to(DEV).contiguous() for k in ("means", "quats", "scales", "opacities")] + [
            sc["sh"].to(DEV) if rgb else None, sc["V"].to(DEV), sc["K"].to(DEV)]
        rc.calibrate(*self.args)
        render, alphas = rc.forward(*self.args)
        rc.check_capacity()
        self.outputs = (render[None].clone(), alphas[None].clone())
        self.full = full_grads

    def grads(self, v, va):
        rc = self.rc
        g = rc.backward(v[0].float().to(DEV).contiguous(), va[0].float().to(DEV).contiguous(), full=self.full)
        rc.check_capacity()
        g = rc.grads_in_input_order(g) if self.full else g
        self.upstream = (v, va)
        return {k: X.f64(t) for k, t in g.items() if t is not None}


@pytest.mark.parametrize("name", list(cam.FUSED_CASES))
def test_fused_path_at_a_skewed_camera(name, monkeypatch):
    _gpu()
    case = cam.FUSED_CASES[name]
    tiny = name.startswith("tiny")
    monkeypatch.setenv("GSLOC_BWD", "tiny" if tiny else "general")
    sc = cam.fused_case(name)
    ctx = case["ctx"]
    want = X.oracle_fused(sc, case["mode"], half=ctx.get("staging") == "fp16", antialiased=ctx.get("antialiased", False))
    got = _HipFused(sc, case)
    rc = got.rc
    assert rc.tiny == tiny, "the context reports another backward than the case names"
    assert (rc.Qh is not None) == (ctx.get("staging") == "fp16") and (rc.vrow is not None) == ctx.get("deterministic", False)
    if not tiny:
        assert int(rc.radii.max()) >= 2
    rows = (rc.row0, rc.row1)
    if "tile_rows" in ctx:
        assert rows == (16, 48)
    figs, flipped, counts, worst, g, _ = X.render_figures(want, got, X.fused_subsets(sc), pose="viewmat", rows=rows)
    tag = f"cameras: fused {name}"
    # pose only (full_grads=False): the same view-matrix gradient from a context that holds no Gaussian gradients
    pose_only = _HipFused(sc, case, full_grads=False)
    assert pose_only.rc.tiny == tiny and torch.equal(pose_only.outputs[0], got.outputs[0])
    g_p = pose_only.grads(*got.upstream)
    assert set(g_p) == {"viewmat"}
    err_p = rel_inf(g_p["viewmat"], g["viewmat"])
    figs["pose-only v_viewmat"] = err_p / POSE_ONLY_TOL
    _report(tag, flipped, figs, counts)
    assert flipped[0] <= X.PIXEL_OUTLIERS, f"{tag}: {flipped[0]:.2e} of the pixels differ from the oracle"
    assert figs["v_viewmat [0]"] < 1.0, (tag, "v_viewmat", figs["v_viewmat [0]"] * POSE_GRAD_TOL)
    assert float(g["viewmat"][3].abs().max()) == 0.0
    assert not failing_subsets(counts), (tag, "outlier Gaussians (count, size, allowed)", counts, worst)
    assert err_p < POSE_ONLY_TOL, (tag, "pose-only v_viewmat against the full backward's", err_p)
    for name_, idx in sc["culled"].items():
        for k in ("means", "quats", "scales", "opacities") if idx else ():
            assert float(g[k][idx].abs().max()) == 0.0, (tag, "a culled row with a gradient", name_, k)


def test_fused_path_drop_in_call_forwards_K_untouched(monkeypatch):
    """rasterization() with one camera and no background at wide_x: the fused path takes it (a cached context appears) and
    its render is the context's, bit for bit."""
    A = _gpu()
    from gsplatloc_amd import fused
    monkeypatch.setenv("GSLOC_BWD", "general")
    monkeypatch.setenv("GSLOC_DISABLE_FUSED", "0")
    monkeypatch.setenv("GSLOC_PACKED", "0")
    monkeypatch.setenv("GSLOC_DROPIN_CACHE", "1")
    name = "general-wide_x"
    sc, case = cam.fused_case(name), cam.FUSED_CASES[name]
    ctx = _HipFused(sc, case, reorder=False)  # (the drop-in call keeps the caller's order of the Gaussians)
    fused.clear_context_cache()
    try:
        r, a, meta = A.rasterization(sc["means"].to(DEV), sc["quats"].to(DEV), sc["scales"].to(DEV), sc["opacities"].to(DEV),
                                     sc["sh"].to(DEV), sc["V"].to(DEV)[None], sc["K"].to(DEV)[None], sc["W"], sc["H"],
                                     sh_degree=1, render_mode=case["mode"], **sc["planes"])
        assert len(fused._CTX_CACHE) == 1 and meta["camera_ids"] is None and meta["isect_ids"] is None
        assert torch.equal(r, ctx.outputs[0]) and torch.equal(a, ctx.outputs[1])
        assert torch.equal(meta["radii"][0], ctx.rc.radii)
    finally:
        fused.clear_context_cache()
