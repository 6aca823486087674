"""Every compositing forward's skip, clamp, stop and last index, per pixel, on the stop-ladder scenes (tests/stop_scenes.py)
against the record-level float64 walk (tests/walk_ref.py) of the records the forward actually used.

Per variant: calibrate and forward a RenderContext, assert that the intended path ran, rebuild the records from the
context, and compare EVERY pixel -- render and alphas at IMAGE_RTOL / IMAGE_ATOL of tests/parity.py, last_ids exactly,
pixels outside the image or the pixel-row window untouched, and for the tiles that are not split the hit lists word for
word.  No pixel is allowed outside: the scenes keep every decision of every pixel at least GPU_MARGIN (1e-3) from its
threshold on those very records, which is asserted first, with its own message ("scene too close to a threshold" is not a
kernel failure).  The largest errors are printed in units of the tolerance.

The staged forward (gsl_rasterize_fwd behind rasterize_to_pixels, csrc/raster.hip: the wave-wide walk) gets the same
records and lists: D = 3 and D = 32, two cameras (the second one holds the records as an fp16-staged record rounds them),
with and without backgrounds; render, alphas and last_ids as above, and t_final RELATIVELY (an absolute bound says nothing
about a T of 1.2e-4).  The t_final bound is 4 x the largest relative error of the reference walk run in float32, in the
reference loop's order, against its float64 run on these scenes -- the kernels associate the product differently -- and
never above 1e-4.  Measured: the float32 walk is within 3.8e-6 (ragged), 5.5e-6 (short), 6.1e-6 (long-c) and 1.2e-5
(long-a) of the float64 one, so the bounds are 1.5e-5 ... 4.7e-5; the staged kernel measured 3.8e-6, 5.5e-6, 6.1e-6 and
1.2e-5 on the MI355X, at its float32 floor.
"""
import functools
import hashlib

import numpy as np
import pytest
import torch

from tests import stop_scenes as S
from tests import walk_ref as WR
from tests.parity import IMAGE_ATOL, IMAGE_RTOL

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -7.0
STRIP = dict(tile_rows=(1, 3), pixel_rows=(19, 39))
VARIANTS = {  # id: (scene, staging, path, render modes)
    "general": ("short", "fp32", "general", ("ED", "RGB+ED", "RGB", "D")),
    "fp16": ("short", "fp16", "general", ("RGB+ED",)),
    "sort-in-forward": ("short", "fp32", "sort-in-forward", ("ED",)),
    "two-pass": ("short", "fp32", "two-pass", ("ED",)),
    "placement": ("short", "fp32", "placement", ("ED",)),
    "strip": ("ragged", "fp32", "strip", ("RGB+ED",)),
    "ragged": ("ragged", "fp32", "general", ("RGB+ED",)),
    **{f"{n}": (n, "fp32", "long", ("ED", "RGB+ED")) for n in S.LONG_SCENES},
    **{f"{n}-fp16": (n, "fp16", "long", ("RGB+ED",)) for n in S.LONG_SCENES},
}
CASES = [pytest.param(v, m, id=f"{v}-{m}") for v, (_, _, _, modes) in VARIANTS.items() for m in modes]
_REF = {}


def _reference(rec, offs, flat, W, H, ed, kw, long_min, seg):
    """The walk of the frame, once per distinct set of records and lists (the fp32 variants of a scene share theirs)."""
    h = hashlib.sha1()
    for k in sorted(rec):
        h.update(np.ascontiguousarray(rec[k]).tobytes())
    h.update(offs.tobytes() + flat.tobytes() + repr((W, H, ed, sorted(kw.items()), long_min, seg)).encode())
    key = h.hexdigest()
    if key not in _REF:
        if len(_REF) > 8:
            _REF.clear()
        _REF[key] = WR.frame_reference(rec, offs, flat, W, H, ed, kw.get("tile_rows"), kw.get("pixel_rows"),
                                       long_min=long_min, seg=seg)
    return _REF[key]


def assert_scene_margin(tag, ref):
    worst = min(float(ref["margin_alpha"].min()), float(ref["margin_T"].min()))
    assert worst >= S.GPU_MARGIN, (f"{tag}: scene too close to a threshold (smallest decision margin {worst:.2e} on the "
                                   f"records the forward used; the scene, not the kernel, needs another nudge)")


@pytest.mark.parametrize("variant,mode", CASES)
def test_every_pixel_decides_as_the_reference_walk(variant, mode, monkeypatch):
    from gsplatloc_amd.context import LONG_MIN, RenderContext
    name, staging, path, _ = VARIANTS[variant]
    sc = S.scene(name)
    W, H, N = sc["W"], sc["H"], sc["N"]
    monkeypatch.setenv("GSLOC_BWD", "general")
    if path == "sort-in-forward":
        monkeypatch.setenv("GSLOC_SORT_IN_FORWARD", "force")
    if path == "two-pass":
        monkeypatch.setenv("GSLOC_BINNING", "two-pass")
    kw = dict(STRIP) if path == "strip" else {}
    rc = RenderContext(N, W, H, mode, sh_degree=None, K_sh=0, device=DEV, full_grads=True, staging=staging,
                       reorder=path == "placement", sort_in_forward=path == "sort-in-forward", **kw)
    ins = S.inputs(sc, mode, DEV)
    rc.calibrate(*ins)
    tag = f"fwd decisions {variant} {mode}"
    # the path ran
    assert not rc.tiny and (rc.Qh is not None) == (staging == "fp16"), tag
    assert (rc.long_min > 0) == (path == "long") and rc.long_min in (0, LONG_MIN), (tag, rc.long_min)
    assert rc.sorts_in_forward() == (path == "sort-in-forward"), tag
    assert (rc.bins is None) == (path == "two-pass"), tag
    assert (rc.order_ids is not None) == (path == "placement"), tag
    rc.render.fill_(SENTINEL)
    rc.alphas.fill_(SENTINEL)
    rc.last_ids.fill_(int(SENTINEL))
    render, alphas = rc.forward(*ins)
    torch.cuda.synchronize()
    rc.check_capacity()
    seg = int(rc.lib.gsl_long_segment())
    if path == "long":
        assert int(rc.long_ws[:16].view(torch.int32)[0]) > 0, "no long-list segment was composited"
    rec, offs, flat = WR.records_from_context(rc)
    if path != "strip":  # the ladder is what it says
        sizes = {t: int(offs[t[1] * rc.tw + t[0] + 1] - offs[t[1] * rc.tw + t[0]]) for t in sc["tiles"]}
        assert sizes == {t: spec["n"] for t, spec in sc["tiles"].items()}, (tag, sizes)
        assert int(offs[-1]) == sum(sizes.values()), tag
    ref = _reference(rec, offs, flat, W, H, rc.ed, kw, rc.long_min, seg)
    assert_scene_margin(tag, ref)
    got = WR.to_numpy_frame(render, alphas, rc.last_ids)
    got["untouched"] = ((got["render"] == SENTINEL).all(-1) & (got["alphas"][..., 0] == SENTINEL)
                        & (got["last_ids"] == int(SENTINEL)))
    got["hits"] = WR.context_hits(rc, offs)
    assert any(len(w) for w in ref["hits"].values()), tag
    fails, figs = WR.compare_frames(got, ref, IMAGE_RTOL, IMAGE_ATOL)
    print(f"[decisions] {tag}: largest error / tolerance: render {figs['render']:.3f}, alphas {figs['alphas']:.3f}; "
          f"smallest margin alpha {ref['margin_alpha'].min():.2e} T {ref['margin_T'].min():.2e}; "
          f"pixels stopped {int((ref['stop'] >= 0).sum())}")
    assert not fails, (tag, fails)


# ---------------------------------------------------------------------------------------------------------------------
# the staged forward
# ---------------------------------------------------------------------------------------------------------------------
T_FINAL_CAP = 1e-4


@functools.lru_cache(maxsize=None)
def _staged_case(name, D):
    """Two cameras over one scene: the records of the float32 oracle projection, plain and half-rounded (both inside the
    scene condition, tests/test_walk_ref_cpu.py), D random features, one list per camera; the float64 walk of both and
    the float32 walk's largest relative t_final error."""
    sc = S.scene(name)
    W, H, N = sc["W"], sc["H"], sc["N"]
    feats = torch.rand(N, D, generator=torch.Generator().manual_seed(D)).double().numpy()
    cams, refs, floor = [], [], 0.0
    for half in (False, True):
        rec, offs, flat = WR.records_from_oracle(sc, "ED", half)
        rec["feat"] = feats
        ref = WR.frame_reference(rec, offs, flat, W, H, False)
        ref32 = WR.frame_reference(rec, offs, flat, W, H, False, dtype=np.float32)
        same = (ref32["last_ids"] == ref["last_ids"]) & (ref32["stop"] == ref["stop"])
        assert same.all(), "the float32 walk decides differently: scene too close to a threshold"
        floor = max(floor, float(np.abs(ref32["T"].astype(np.float64) / ref["T"] - 1.0).max()))
        cams.append((rec, offs, flat))
        refs.append(ref)
    return sc, cams, refs, floor


@pytest.mark.parametrize("background", [False, True], ids=["no-background", "background"])
@pytest.mark.parametrize("D", [3, 32])
@pytest.mark.parametrize("name", ["short", "ragged", "long-a", "long-c"])
def test_staged_forward_decides_as_the_reference_walk(name, D, background):
    """rasterize_to_pixels' forward: render, alphas, last_ids per pixel, and t_final within 4 x the float32 walk's own
    error (measured 3.8e-6 ... 1.2e-5 on these scenes, the kernel the same: bounds 1.5e-5 ... 4.7e-5; never above 1e-4)."""
    import gsplatloc_amd as A
    sc, cams, refs, floor = _staged_case(name, D)
    W, H, N = sc["W"], sc["H"], sc["N"]
    tw, th = (W + 15) // 16, (H + 15) // 16
    f = lambda key: torch.tensor(np.stack([c[0][key] for c in cams]), dtype=torch.float32, device=DEV)  # noqa: E731
    means2d = torch.stack([f("x"), f("y")], -1).contiguous()
    conics = torch.stack([f("a"), f("b"), f("c")], -1).contiguous()
    colors = f("feat").contiguous().requires_grad_()
    n0 = int(cams[0][2].shape[0])
    flat = torch.tensor(np.concatenate([cams[0][2], cams[1][2] + N]), dtype=torch.int32, device=DEV)
    offsets = torch.tensor(np.stack([cams[0][1][:-1], cams[1][1][:-1] + n0]), dtype=torch.int32, device=DEV).reshape(2, th, tw)
    bg = torch.rand(2, D, generator=torch.Generator().manual_seed(1)) if background else None
    render, alphas = A.rasterize_to_pixels(means2d, conics, colors, f("op"), W, H, 16, offsets, flat,
                                           backgrounds=bg.to(DEV) if background else None)
    torch.cuda.synchronize()
    last_ids, t_final = render.grad_fn.saved_tensors[-2:]
    assert last_ids.dtype == torch.int32 and t_final.shape == (2, H, W)
    bound = min(T_FINAL_CAP, 4.0 * floor)
    for c in range(2):
        ref = dict(refs[c])
        tag = f"staged {name} D={D} camera {c} background={background}"
        assert_scene_margin(tag, ref)
        if background:
            ref["render"] = ref["render"] + ref["T"][..., None] * bg[c].double().numpy()
        ref["last_ids"] = np.where(ref["n"] > 0, ref["last_ids"] + (n0 if c else 0), 0)
        got = WR.to_numpy_frame(render[c], alphas[c], last_ids[c])
        fails, figs = WR.compare_frames(got, ref, IMAGE_RTOL, IMAGE_ATOL, hits=False)
        rel = float(np.abs(t_final[c].cpu().double().numpy() / ref["T"] - 1.0).max())
        print(f"[decisions] {tag}: largest error / tolerance: render {figs['render']:.3f}, alphas {figs['alphas']:.3f}; "
              f"t_final relative {rel:.2e} (float32 walk {floor:.2e}, bound {bound:.2e})")
        assert not fails, (tag, fails)
        assert rel <= bound, (tag, "t_final", rel, bound)
