"""Every gradient path in a moved world: the ladder scene of tests/test_gpu_grad_paths.py built at dataset-scale cameras.

The product tracks in the PCA frame of the target cloud (data/normalize.py): an arbitrary rotation, mostly with a negative
trace, and translations of metres.  The ladder scene is built on screen and back-projected through its camera, so at a
far camera the same tile lists appear with world coordinates metres off the origin and a dense rotation: means R + t,
campos = -R^T t, the SH view directions and the lever arms of v_R all cancel differently in float32.

The comparison is run_path_case() of test_gpu_grad_paths.py with its assertions as they are.  One bound may differ, for
a float32 reason: with lever arms of metres the view-matrix gradient of a float32 pipeline can sit above 1e-4 of its
largest entry.  A case that misses POSE_GRAD_TOL measures the floor -- the oracle itself run in float32 on the same
float32 inputs and the same upstream gradient, against its float64 run -- prints it, bounds it by parity.FLOOR32_MAX,
and allows max(POSE_GRAD_TOL, 1.25 x floor), the rule of parity.pose_grad_bound.
"""
import pytest
import torch

from tests.grad_paths import compare_grads, failing_subsets, oracle_render, roll_within
from tests.parity import FLOOR32_MAX, POSE_GRAD_TOL, agreeing_pixels, rel_inf, report
from tests.pose_ref import far_poses
from tests.scenes import small_pose
from tests.test_gpu_grad_paths import (DEV, MAX_FLIPPED, NAMES, H, W, _ladder_scene, _oracle, _oracle_grads, _upstream,
                                       pose_key, run_path_case)

pytestmark = pytest.mark.gpu

# not axis-aligned with the world: the far pose composed with a small seeded one
CAMERAS = {name: pose_key(far_poses()[name] @ small_pose(0.4, 0.01)) for name in ("m00", "m22")}
# RGB+ED renders SH degree 1 with the scene's non-zero higher coefficients: v_campos != 0
MATRIX = [("general", "RGB+ED", "random"), ("general", "RGB+ED", "tracker"), ("deterministic", "RGB+ED", "random"),
          ("placement", "RGB+ED", "random"), ("strip", "RGB+ED", "random"), ("general", "ED", "random"),
          ("fp16-general", "RGB+ED", "random"), ("tiny", "RGB+ED", "random"), ("long", "ED", "random")]


def _float32_floor(tag, sc, mode, half, oracle, v, va):
    """The view-matrix gradient of the oracle run in float32 against its float64 run, relative to the largest entry;
    returns the bound of the comparison.  Flip-aware like every comparison here (tests/parity.py): a pixel on which the
    float32 oracle takes another compositing decision than the float64 one is left out on both sides -- one such pixel
    of 27 200 is worth 3e-4 to 6e-3 of the gradient, and which pixel flips changes with the host's libm."""
    leaves64, r_o, a_o = oracle
    sh = 1 if mode in ("RGB+ED", "RGB+D") else None
    leaves = [sc[k].clone().requires_grad_() for k in ("means", "quats", "scales", "opacities")]
    colors = None
    if mode.startswith("RGB"):
        colors = (sc["sh"] if sh is not None else sc["rgb"]).clone().requires_grad_()
    V = sc["V"].clone().requires_grad_()
    r, a = oracle_render(*leaves, colors, V, sc["K"], W, H, mode, sh_degree=sh, half=half)
    ok = agreeing_pixels(r.detach().double(), a.detach().double(), r_o.detach(), a_o.detach())
    v, va = v * ok[..., None], va * ok[..., None]
    want = _oracle_grads(oracle, v, va)
    (gv,) = torch.autograd.grad([r, a], [V], grad_outputs=[v.float(), va.float()])
    floor = rel_inf(gv[:3], want["viewmat"][:3])
    report(tag + " float32 oracle", 1.0 - ok.double().mean().item(), v_viewmat_floor=floor)
    assert floor <= FLOOR32_MAX, (tag, "the float32 floor itself is out of bounds", floor)
    return max(POSE_GRAD_TOL, 1.25 * floor)


def _far_cases():
    out = []
    for cam in CAMERAS:
        for path, mode, up in MATRIX:
            out.append(pytest.param(cam, path, mode, up, id=f"{cam}-{path}-{mode}-{up}"))
    return out


def test_far_cameras_are_far():
    for name, key in CAMERAS.items():
        c2w = torch.tensor(key, dtype=torch.float64).reshape(4, 4)
        assert float(c2w[:3, :3].trace()) < 0 and float(c2w[:3, 3].norm()) > 3.0
        assert float(c2w[:3, :3].abs().min()) > 1e-3  # dense
        sc = _ladder_scene("ladder", key)
        assert float(sc["means"].abs().max()) > 5.0
        assert torch.equal(_ladder_scene("ladder")["opacities"], sc["opacities"])  # the same ladder on screen


@pytest.mark.parametrize("camera,path,mode,upstream", _far_cases())
def test_gradient_paths_at_far_cameras(camera, path, mode, upstream, monkeypatch):
    run_path_case(path, mode, upstream, monkeypatch, c2w=CAMERAS[camera], label=f"far pose {camera}",
                  pose_tol=_float32_floor)


@pytest.mark.parametrize("via", ["staged", "packed"])
def test_rasterization_staged_and_packed_at_a_far_camera(via, monkeypatch):
    """rasterization() with the fused path off -- gsl_project_fwd/bwd, gsl_sh_*, gsl_rasterize_* -- and with
    packed=True (gsl_project_packed_*), on the m22 scene: every input gradient against the oracle."""
    import gsplatloc_amd as A
    monkeypatch.setenv("GSLOC_DISABLE_FUSED", "1")
    monkeypatch.setenv("GSLOC_PACKED", "1" if via == "packed" else "0")
    # the path ran: the fused entry points are barred, the staged / packed projection launches are counted
    import gsplatloc_amd.rendering as rendering
    from gsplatloc_amd._lib import load_library

    def barred(*a, **k):
        raise AssertionError("the fused path was taken")

    for name in ("cached_rasterization", "fused_rasterization", "fused_absgrad_rasterization"):
        monkeypatch.setattr(rendering, name, barred)
    lib, launches = load_library(), {}
    for name in ("gsl_project_fwd", "gsl_project_packed_fill", "gsl_rasterize_fwd", "gsl_sh_fwd"):
        def counted(*a, _f=getattr(lib, name), _n=name):
            launches[_n] = launches.get(_n, 0) + 1
            return _f(*a)
        monkeypatch.setattr(lib, name, counted)
    key, mode = CAMERAS["m22"], "RGB+ED"
    sc = _ladder_scene("ladder", key)
    ins = dict(means=sc["means"], quats=sc["quats"], scales=sc["scales"], opacities=sc["opacities"], colors=sc["sh"],
               viewmats=sc["V"][None])
    ins = {k: t.to(DEV).clone().requires_grad_() for k, t in ins.items()}
    render, alphas, meta = A.rasterization(**ins, Ks=sc["K"][None].to(DEV), width=W, height=H, sh_degree=1,
                                           render_mode=mode, packed=via == "packed", near_plane=0.01, far_plane=1e10,
                                           rasterize_mode="classic")
    assert (meta.get("camera_ids") is not None) == (via == "packed")
    assert launches.get("gsl_rasterize_fwd", 0) >= 1 and launches.get("gsl_sh_fwd", 0) >= 1, launches
    assert ("gsl_project_packed_fill" in launches) == (via == "packed"), launches
    assert ("gsl_project_fwd" in launches) == (via == "staged"), launches
    leaves, r_o, a_o = _oracle("ladder", mode, False, key)
    rg, ag = render[0].detach().cpu().double(), alphas[0].detach().cpu().double()
    ok = agreeing_pixels(rg, ag, r_o.detach(), a_o.detach())
    flipped = 1.0 - ok.double().mean().item()
    tag = f"far pose m22 rasterization() {via}"
    assert flipped <= MAX_FLIPPED, f"{tag}: {flipped:.2e} of the pixels differ from the oracle"
    v, va = _upstream("random", 4, ok)
    want = _oracle_grads((leaves, r_o, a_o), v, va)
    torch.autograd.backward([render, alphas], [v.float().to(DEV)[None], va.float().to(DEV)[None]])
    got = {nm: ins[nm].grad for nm in NAMES}
    ref = {nm: want[nm] for nm in NAMES}
    worst, counts, _ = compare_grads(got, ref, sc["subsets"])
    for nm in NAMES:
        assert float(got[nm].cpu()[sc["culled"]].abs().max()) == 0.0, (tag, "culled Gaussian with a gradient", nm)
    _, rolled, _ = compare_grads(roll_within(got, sc["groups"]), ref, sc["subsets"])
    err_v = rel_inf(ins["viewmats"].grad[0, :3], want["viewmat"][:3])
    report(tag, flipped, v_viewmat=err_v, **{"v_" + k: x for k, x in worst.items()},
           **{"outliers " + k: float(c[0]) for k, c in counts.items()})
    tol = POSE_GRAD_TOL if err_v < POSE_GRAD_TOL else _float32_floor(tag, sc, mode, False, (leaves, r_o, a_o), v, va)
    assert err_v < tol, (tag, err_v, tol)
    assert not failing_subsets(counts), (tag, counts, worst)
    assert set(failing_subsets(rolled)) == set(counts), (tag, "rolled rows not rejected in every subset", rolled)
