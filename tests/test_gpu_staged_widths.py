"""The staged route's gradients at every channel width and camera count, against the float64 oracle.

rasterization() leaves the fused route for several cameras, a background, feature vectors, packed / sparse gradients and
GSLOC_DISABLE_FUSED=1; the stage operators then run k_raster_fwd/bwd<D> for D in ops.SUPPORTED_CHANNELS, the accumulator
rows of 16 or 48 floats behind them (gsl_vacc_bytes, gsl_vacc_unpack) and, for absgrad, k_absgrad<D, false, false>
(tests/test_gpu_absgrad.py has those cases).  Here:

  1. rasterize_to_pixels alone at every width (and the padded ones), with and without a background, one and two cameras:
     render, alpha, the four per-row gradients, their sums, v_backgrounds; on the sparse scene the rows nothing touches
     and the empty tile;
  2. gsl_rasterize_bwd + gsl_vacc_unpack called directly between sentinel rows;
  3. rasterization() end to end: 33 channels in chunks of 32 and of 7 (dense, GSLOC_PACKED=1, sparse_grad), 16 channels
     antialiased, per-camera SH coefficients and colours, 2 channels; every input gradient, v_viewmats per camera,
     v_backgrounds.

Scenes and their conditions: tests/staged_widths.py, tests/test_staged_widths_cpu.py.  Every comparison is with
oracle/gsplat_oracle.py in float64 on the same float32 inputs, flip-aware as tests/parity.py describes; the bounds are
those of tests/grad_paths.py, test_fused_full_gradients and test_rasterize_fwd_bwd, unchanged.

What these tests found: on the deep scene every pixel ends at a transmittance of 1e-4 .. 1e-2, and a backward that starts
from T = 1 - render_alphas (float32) has T to 3e-8 absolute only, 3e-4 relative.  The summed gradients reached 8e-3 and
v_viewmats 5e-4 of their largest entry; with the forward's own T handed to the backward (gsl_rasterize_fwd's t_final) they
are at 1e-6 .. 8e-5 and 3e-6 (NOTES.md has the figures).
"""
import functools

import pytest
import torch

from oracle import gsplat_oracle as G
from tests import staged_widths as S
from tests.grad_paths import compare_grads, failing_subsets, roll_within
from tests.parity import IMAGE_ATOL, IMAGE_RTOL, POSE_GRAD_TOL, agreeing_pixels, rel_inf, report

pytestmark = pytest.mark.gpu

DEV = "cuda"
MAX_FLIPPED = 3e-3  # pixels sitting on a compositing threshold (test_fused_full_gradients' bound)
SUM_TOL = 5e-4      # gradients summed over the Gaussians (test_rasterize_fwd_bwd, test_fused_full_gradients)
WIDTHS = (1, 2, 3, 4, 5, 8, 16, 32)
STAGE = ("means2d", "conics", "colors", "opacities")
SENTINEL, GUARD_ROWS = -7.25, 64


def _gpu():
    import gsplatloc_amd as A
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert A.ops.SUPPORTED_CHANNELS == WIDTHS
    return A


def _agree(r_g, a_g, r_o, a_o):
    ok = agreeing_pixels(r_g, a_g, r_o.detach(), a_o.detach(), rtol=IMAGE_RTOL, atol=IMAGE_ATOL)
    return ok, 1.0 - ok.double().mean().item()


@functools.lru_cache(maxsize=None)
def _walk(scene, C):
    st = S.stage_inputs(scene, C, 1)
    return S.walk(st["means2d"], st["conics"], st["opacities"], st["offsets"], st["flatten_ids"])


def _stage_oracle(st, with_bg):
    """float64 forward of the oracle on the float32 stage inputs: (leaves, render, alphas)."""
    names = STAGE + (("backgrounds",) if with_bg else ())
    leaves = {k: st[k].double().clone().requires_grad_() for k in names}
    rc, ra = G.rasterize_to_pixels(*[leaves[k] for k in STAGE], S.W, S.H, 16, st["offsets"], st["flatten_ids"],
                                   backgrounds=leaves.get("backgrounds"))
    return leaves, rc, ra


def _stage_ours(A, st, with_bg):
    ins = {k: st[k].to(DEV).clone().requires_grad_() for k in STAGE}
    if with_bg:
        ins["backgrounds"] = st["backgrounds"].to(DEV).clone().requires_grad_()
    rc, ra = A.rasterize_to_pixels(*[ins[k] for k in STAGE], S.W, S.H, 16, st["offsets"].to(DEV),
                                   st["flatten_ids"].to(DEV), backgrounds=ins.get("backgrounds"))
    assert rc.shape == (st["C"], S.H, S.W, st["D"]) and ra.shape == (st["C"], S.H, S.W, 1)
    return ins, rc, ra


def _backward(rc, ra, v, va):
    ((rc * v.float().to(DEV)).sum() + (ra * va.float().to(DEV)).sum()).backward()
    torch.cuda.synchronize()


def _check_backgrounds(tag, got, want):
    """v_backgrounds [C,D] within POSE_GRAD_TOL of its largest entry; the same with its channels rolled is rejected."""
    err = rel_inf(got, want)
    assert err < POSE_GRAD_TOL, (tag, "v_backgrounds", err)
    if want.shape[-1] > 1:
        assert rel_inf(got.roll(1, -1), want) >= POSE_GRAD_TOL, (tag, "v_backgrounds with rolled channels not rejected")
    return err


def _stage_cases():
    out = [(D, 1, bg) for D in WIDTHS + tuple(S.PADDED) for bg in (False, True)]
    out += [(D, 2, bg) for D in (5, 16, 32) for bg in (False, True)]
    return [pytest.param(*c, id=f"D{c[0]}-C{c[1]}-{'bg' if c[2] else 'nobg'}") for c in out]


@pytest.mark.parametrize("D,C,with_bg", _stage_cases())
def test_stage_compositing_at_every_width(D, C, with_bg):
    """rasterize_to_pixels on the deep scene: every k_raster_fwd / k_raster_bwd instantiation, lists of two to five
    batches that the pixels walk to the end or leave on the T threshold."""
    A = _gpu()
    assert A.ops._pad_channels(D) == S.PADDED.get(D, D)
    st, wk = S.stage_inputs("deep", C, D), _walk("deep", C)
    leaves, rc_o, ra_o = _stage_oracle(st, with_bg)
    ins, rc_g, ra_g = _stage_ours(A, st, with_bg)
    ok, flipped = _agree(rc_g, ra_g, rc_o, ra_o)
    tag = f"staged widths stage D={D} C={C} bg={int(with_bg)}"
    v, va = S.upstream(rc_o.shape, ra_o.shape, ok)
    want = S.oracle_grads(leaves, (rc_o, ra_o), (v, va))
    _backward(rc_g, ra_g, v, va)
    got = S.flat_rows({k: ins[k].grad.cpu() for k in STAGE})
    ref = S.flat_rows({k: want[k] for k in STAGE})
    subsets = {"all": (st["radii"].reshape(-1) > 0).nonzero()[:, 0], "past the first batch": wk["late"].nonzero()[:, 0]}
    worst, counts, _ = compare_grads(got, ref, subsets)
    _, rolled, _ = compare_grads(roll_within(got, S.tile_groups(st["means2d"], st["radii"])), ref, subsets)
    sums = {k: rel_inf(ins[k].grad.sum(1), want[k].sum(1)) for k in STAGE}
    err_bg = rel_inf(ins["backgrounds"].grad, want["backgrounds"]) if with_bg else 0.0
    report(tag, flipped, v_backgrounds=err_bg, **{"v_" + k: x for k, x in worst.items()},
           **{"sum v_" + k: x for k, x in sums.items()}, **{"outliers " + k: float(c[0]) for k, c in counts.items()},
           **{"rolled outliers " + k: float(c[0]) for k, c in rolled.items()})
    assert flipped <= MAX_FLIPPED, f"{tag}: {flipped:.2e} of the pixels differ from the oracle"
    assert not failing_subsets(counts), (tag, "outlier rows (count, size, allowed)", counts, worst)
    assert set(failing_subsets(rolled)) == set(counts), (tag, "rolled rows not rejected in every subset", rolled)
    for k in STAGE:
        assert sums[k] < SUM_TOL, (tag, k + " (summed)", sums[k])
    if with_bg:
        _check_backgrounds(tag, ins["backgrounds"].grad, want["backgrounds"])


@pytest.mark.parametrize("with_bg", [False, True], ids=["nobg", "bg"])
@pytest.mark.parametrize("D", WIDTHS + tuple(S.PADDED))
def test_untouched_rows_and_the_empty_tile_at_every_width(D, with_bg):
    """The sparse scene: culled and never-composited Gaussians get gradient rows of exactly zero, the empty tile renders
    the background (or 0) with alpha exactly 0; the rest of the frame and the composited rows match the oracle."""
    A = _gpu()
    sc, st, wk = S.sparse_scene(), S.stage_inputs("sparse", 1, D), _walk("sparse", 1)
    leaves, rc_o, ra_o = _stage_oracle(st, with_bg)
    ins, rc_g, ra_g = _stage_ours(A, st, with_bg)
    ok, flipped = _agree(rc_g, ra_g, rc_o, ra_o)
    tag = f"staged widths sparse D={D} bg={int(with_bg)}"
    assert flipped <= MAX_FLIPPED, f"{tag}: {flipped:.2e} of the pixels differ from the oracle"
    tx, ty = S.EMPTY_TILE
    tile_c = rc_g.detach()[0, 16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16].cpu()
    tile_a = ra_g.detach()[0, 16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16].cpu()
    fill = st["backgrounds"][0] if with_bg else torch.zeros(D)
    assert torch.equal(tile_c, fill.expand_as(tile_c).contiguous()), (tag, "empty tile")
    assert float(tile_a.abs().max()) == 0.0, (tag, "empty tile's alpha")
    v, va = S.upstream(rc_o.shape, ra_o.shape, ok)
    want = S.oracle_grads(leaves, (rc_o, ra_o), (v, va))
    _backward(rc_g, ra_g, v, va)
    zero = torch.cat([sc["culled"], sc["faint"], sc["edge"]])
    composited = wk["composited"].nonzero()[:, 0]
    assert composited.numel() == S.N_PLAIN
    for k in STAGE:
        g = ins[k].grad[0].cpu()
        assert float(g[zero].abs().max()) == 0.0, (tag, "a row that nothing composites has a gradient", k)
    got = S.flat_rows({k: ins[k].grad.cpu() for k in STAGE})
    worst, counts, _ = compare_grads(got, S.flat_rows({k: want[k] for k in STAGE}), {"composited": composited})
    assert not failing_subsets(counts), (tag, counts, worst)
    if with_bg:
        _check_backgrounds(tag, ins["backgrounds"].grad, want["backgrounds"])


@pytest.mark.parametrize("D", [5, 8, 16, 32])
def test_accumulator_rows_through_the_c_entry_points(D):
    """gsl_rasterize_bwd + gsl_vacc_unpack called directly: rows of 16 floats up to 10 channels and of 48 beyond, nothing
    written behind the accumulator or behind the four outputs, and the values rasterize_to_pixels' backward returns."""
    A = _gpu()
    from gsplatloc_amd import _lib
    lib, ptr, stream = _lib.load_library(), _lib.ptr, _lib.current_stream()
    st = S.stage_inputs("deep", 1, D)
    n = st["N"]
    dev = lambda t: t.to(DEV).contiguous()  # noqa: E731
    m2, con, col, opa = (dev(st[k][0]) for k in STAGE)
    bg = dev(st["backgrounds"][0])
    fl = dev(st["flatten_ids"].to(torch.int32))
    n_isects = fl.numel()
    offs = dev(torch.cat([st["offsets"].reshape(-1).to(torch.int32), torch.tensor([n_isects], dtype=torch.int32)]))
    assert offs.numel() == S.TW * S.TH + 1 and int(offs.max()) == n_isects and int(fl.max()) < n and int(fl.min()) >= 0
    rc = torch.empty(S.H, S.W, D, device=DEV)
    ra = torch.empty(S.H, S.W, 1, device=DEV)
    last = torch.empty(S.H, S.W, dtype=torch.int32, device=DEV)
    tf = torch.full((S.H + GUARD_ROWS, S.W), SENTINEL, device=DEV)
    _lib.check(lib.gsl_rasterize_fwd(ptr(m2), ptr(con), ptr(col), ptr(opa), ptr(bg), D, S.W, S.H, 16, S.TW, S.TH, 0, S.TH,
                                     ptr(offs), ptr(fl), n_isects, ptr(rc), ptr(ra), ptr(last), ptr(tf), stream),
               "gsl_rasterize_fwd")
    gen = torch.Generator().manual_seed(7)
    v = dev(torch.randn(S.H, S.W, D, generator=gen))
    va = dev(torch.randn(S.H, S.W, 1, generator=gen))
    stride = 16 if D <= 10 else 48
    assert lib.gsl_vacc_bytes(n, D) == n * stride * 4
    vacc = torch.full(((n + GUARD_ROWS) * stride,), SENTINEL, device=DEV)
    vacc[:n * stride] = 0.0
    outs = {k: torch.full((n + GUARD_ROWS,) + tuple(t.shape[1:]), SENTINEL, device=DEV)
            for k, t in zip(STAGE, (m2, con, col, opa))}
    _lib.check(lib.gsl_rasterize_bwd(ptr(m2), ptr(con), ptr(col), ptr(opa), ptr(bg), D, S.W, S.H, 16, S.TW, S.TH, 0, S.TH,
                                     ptr(offs), ptr(fl), n_isects, ptr(ra), ptr(last), ptr(tf), ptr(v), ptr(va), ptr(vacc),
                                     stream), "gsl_rasterize_bwd")
    _lib.check(lib.gsl_vacc_unpack(ptr(vacc), n, D, ptr(outs["means2d"]), ptr(outs["conics"]), ptr(outs["colors"]),
                                   ptr(outs["opacities"]), stream), "gsl_vacc_unpack")
    torch.cuda.synchronize()
    assert bool((vacc[n * stride:] == SENTINEL).all()), "write behind the accumulator rows"
    assert bool((tf[S.H:] == SENTINEL).all()), "write behind t_final"
    # t_final is the T that the alpha image was rounded from (nothing composites down to the float32 1e-4 stop or below)
    assert torch.equal(1.0 - tf[:S.H], ra[..., 0]) and float(tf[:S.H].min()) > 0.9999e-4
    assert float(vacc[:n * stride].view(n, stride)[:, 6 + D:].abs().max()) == 0.0, "write into a row's padding"
    for k, t in outs.items():
        assert bool((t[n:] == SENTINEL).all()), f"write behind v_{k}"
        assert bool(torch.isfinite(t[:n]).all()) and not bool((t[:n] == SENTINEL).any()), k
    # the same inputs through the autograd operator
    ins = {k: t[None].clone().requires_grad_() for k, t in zip(STAGE, (m2, con, col, opa))}
    rc_a, ra_a = A.rasterize_to_pixels(*[ins[k] for k in STAGE], S.W, S.H, 16, dev(st["offsets"]), fl, backgrounds=bg[None])
    assert torch.equal(rc_a[0], rc) and torch.equal(ra_a[0], ra)
    ((rc_a[0] * v).sum() + (ra_a[0] * va).sum()).backward()
    for k in STAGE:
        err = rel_inf(outs[k][:n], ins[k].grad[0])
        assert err < 1e-6, (k, err)  # two orders of the same float32 atomic sums


# ---- rasterization() end to end -----------------------------------------------------------------------------------------
_E2E = {}


def _e2e_oracle(name):
    """The oracle's forward of a case and its walk (kept for the next test of the same case)."""
    if name not in _E2E:
        _E2E.clear()
        ins, Ks, kw = S.e2e_inputs(name)
        leaves, r, a, meta = S.oracle_e2e(ins, Ks, kw)
        wk = S.walk(meta["means2d"].detach(), meta["conics"].detach(), meta["opacities"].detach(), meta["isect_offsets"],
                    meta["flatten_ids"])
        _E2E[name] = (ins, Ks, kw, leaves, r, a, meta, wk)
    return _E2E[name]


def _e2e_cases():
    out = [("c3-33ch", route, chunk) for chunk in (32, 7) for route in ("staged", "sparse", "env")]
    out += [(name, "staged", 32) for name in S.E2E_CASES if name != "c3-33ch"]
    return [pytest.param(*c, id=f"{c[0]}-{c[1]}-chunk{c[2]}") for c in out]


@pytest.mark.parametrize("name,route,chunk", _e2e_cases())
def test_rasterization_on_the_staged_route(name, route, chunk, monkeypatch):
    """rasterization() with the fused route off: dense ("staged"), packed with dense gradients ("env": GSLOC_PACKED=1)
    and packed with sparse gradients ("sparse"), all three against the oracle."""
    A = _gpu()
    monkeypatch.setenv("GSLOC_DISABLE_FUSED", "1")
    monkeypatch.setenv("GSLOC_PACKED", "1" if route == "env" else "0")
    ins, Ks, kw, leaves, r_o, a_o, meta_o, wk = _e2e_oracle(name)
    case = S.E2E_CASES[name]
    C, n = case["C"], ins["means"].shape[0]
    ins_g = {k: t.to(DEV).clone().requires_grad_() for k, t in ins.items() if t is not None}
    r_g, a_g, meta = A.rasterization(ins_g["means"], ins_g["quats"], ins_g["scales"], ins_g["opacities"], ins_g["colors"],
                                     ins_g["viewmats"], Ks.to(DEV), backgrounds=ins_g.get("backgrounds"),
                                     packed=route != "staged", sparse_grad=route == "sparse", channel_chunk=chunk, **kw)
    assert r_g.shape == r_o.shape and a_g.shape == a_o.shape
    assert (meta["camera_ids"] is None) == (route == "staged")  # the route ran
    if route == "staged":
        assert meta["means2d"].shape == (C, n, 2) and "Q0" not in meta
    ok, flipped = _agree(r_g, a_g, r_o, a_o)
    tag = f"staged widths e2e {name} {route} chunk={chunk}"
    v, va = S.upstream(r_o.shape, a_o.shape, ok)
    want = S.oracle_grads(leaves, (r_o, a_o), (v, va))
    _backward(r_g, a_g, v, va)
    got = {k: (t.grad.to_dense() if t.grad.is_sparse else t.grad).cpu() for k, t in ins_g.items()}
    if route == "sparse":
        assert ins_g["means"].grad.is_sparse and not ins_g["viewmats"].grad.is_sparse
    # v_viewmats, camera by camera; the neighbour camera's gradient in its place is rejected
    # (the whole matrix: the oracle's last row is zero, and so must ours be)
    err_v = [rel_inf(got["viewmats"][c], want["viewmats"][c]) for c in range(C)]
    swapped = [rel_inf(got["viewmats"][(c + 1) % C], want["viewmats"][c]) for c in range(C)]
    # per Gaussian: the inputs shared by the cameras, then per-camera colours row by row
    seen = (meta_o["radii"] > 0).any(0)
    late = wk["late"].reshape(C, n).any(0)
    shared = [k for k in S.E2E_NAMES if not (k == "colors" and case["per_cam"])]
    worst, counts, _ = compare_grads({k: got[k] for k in shared}, {k: want[k] for k in shared},
                                     {"all": seen.nonzero()[:, 0], "past the first batch": late.nonzero()[:, 0]})
    sums = {k: rel_inf(got[k].sum(0), want[k].sum(0)) for k in shared}
    if case["per_cam"]:
        w2, c2, _ = compare_grads(S.flat_rows({"colors": got["colors"]}), S.flat_rows({"colors": want["colors"]}),
                                  {"all (camera, Gaussian)": (meta_o["radii"].reshape(-1) > 0).nonzero()[:, 0],
                                   "past the first batch (camera, Gaussian)": wk["late"].nonzero()[:, 0]})
        worst.update(w2)
        counts.update(c2)
        sums["colors"] = rel_inf(got["colors"].sum(1), want["colors"].sum(1))
    err_bg = rel_inf(got["backgrounds"], want["backgrounds"]) if case["bg"] else 0.0
    report(tag, flipped, v_viewmats=max(err_v), v_backgrounds=err_bg, **{"v_" + k: x for k, x in worst.items()},
           **{"sum v_" + k: x for k, x in sums.items()}, **{"outliers " + k: float(c[0]) for k, c in counts.items()})
    assert flipped <= MAX_FLIPPED, f"{tag}: {flipped:.2e} of the pixels differ from the oracle"
    for c in range(C):
        assert err_v[c] < POSE_GRAD_TOL, (tag, "v_viewmats of camera", c, err_v[c])
        if C > 1:
            assert swapped[c] >= POSE_GRAD_TOL, (tag, "swapped cameras not rejected", c, swapped[c])
    assert not failing_subsets(counts), (tag, "outlier Gaussians (count, size, allowed)", counts, worst)
    for k, x in sums.items():
        assert x < SUM_TOL, (tag, k + " (summed)", x)
    if case["bg"]:
        _check_backgrounds(tag, got["backgrounds"], want["backgrounds"])
    if case["feat"] is None:  # SH coefficients [C,N,16,3] at degree 2: the seven unused bands get exactly nothing
        used = (S.SH_DEGREE + 1) ** 2
        assert float(got["colors"][:, :, used:].abs().max()) == 0.0, (tag, "gradient in an unused SH band")
        assert float(got["colors"][:, :, :used].abs().amax((0, 1, 3)).min()) > 0.0
