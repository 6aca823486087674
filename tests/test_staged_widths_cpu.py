"""The scenes of tests/test_gpu_staged_widths.py, checked with the oracle alone: the conditions the GPU tests rely on
(list lengths, where the pixels stop, empty tiles, culled and never-composited Gaussians), and that the oracle's own
float32 build stays inside every bound those tests hold the HIP kernels to -- so that a bound missed on the GPU is the
kernels' doing, not the scene's."""
import pytest
import torch

from oracle import gsplat_oracle as G
from tests import staged_widths as S
from tests.grad_paths import compare_grads, failing_subsets
from tests.parity import POSE_GRAD_TOL, agreeing_pixels, rel_inf

MAX_FLIPPED = 3e-3
SUM_TOL = 5e-4
STAGE_NAMES = ("means2d", "conics", "colors", "opacities")


def _walk(st):
    return S.walk(st["means2d"], st["conics"], st["opacities"], st["offsets"], st["flatten_ids"])


def _stage_oracle(st, dtype):
    leaves = {k: st[k].to(dtype).clone().requires_grad_() for k in STAGE_NAMES + ("backgrounds",)}
    rc, ra = G.rasterize_to_pixels(*[leaves[k] for k in STAGE_NAMES], S.W, S.H, 16, st["offsets"], st["flatten_ids"],
                                   backgrounds=leaves["backgrounds"])
    return leaves, rc, ra


def test_deep_scene_walks_several_batches_and_stops_on_the_threshold():
    st = S.stage_inputs("deep", 3, 4)
    wk = _walk(st)
    _, _, ra = _stage_oracle(st, torch.float64)
    assert float((wk["alphas"] - ra[..., 0].detach()).abs().max()) < 1e-12, "walk() is not the oracle's walk"
    for c in range(3):
        lengths = wk["lengths"][c]
        assert int(lengths.min()) > S.BATCH, lengths
        assert int(lengths.max()) > 3 * S.BATCH, lengths
        assert int(wk["last_pos"][c].min()) >= S.BATCH, "a pixel ends inside the first batch"
        assert float((wk["last_pos"][c] >= 2 * S.BATCH).double().mean()) >= 0.5
        stopped = float(wk["stopped"][c].double().mean())
        assert 0.2 <= stopped <= 0.8, stopped
    late = int(wk["late"].sum())
    assert late >= 3 * 100, late  # the subset "composited past the first batch" is large enough for a 1 % count
    assert float(st["opacities"].max()) < 0.999  # no clamped alpha


def test_sparse_scene_has_an_empty_tile_and_rows_nothing_touches():
    sc = S.sparse_scene()
    st = S.stage_inputs("sparse", 1, 3)
    wk = _walk(st)
    _, _, ra = _stage_oracle(st, torch.float64)
    assert float((wk["alphas"] - ra[..., 0].detach()).abs().max()) < 1e-12
    tx, ty = S.EMPTY_TILE
    assert int(wk["lengths"][0, ty, tx]) == 0
    assert int((wk["lengths"][0] > 0).sum()) == S.TW * S.TH - 1
    culled = (st["radii"][0] == 0).nonzero()[:, 0]
    assert torch.equal(culled, sc["culled"]) and culled.numel() == S.N_BEHIND + S.N_OFF
    never = ((st["radii"][0] > 0) & ~wk["composited"]).nonzero()[:, 0]
    assert torch.equal(never, torch.cat([sc["faint"], sc["edge"]])) and never.numel() == S.N_FAINT + S.N_EDGE >= 10
    # ... by a margin that float32 cannot cross, and in a list each; every other visible row is composited
    assert float(wk["amax"][never].min()) >= 0.0 and float(wk["amax"][never].max()) < 0.75 * G.ALPHA_MIN
    assert int(wk["composited"].sum()) == S.N_PLAIN
    assert not bool(wk["stopped"].any())
    # the float32 build of the oracle keeps these rows at exactly zero and the empty tile at alpha 0
    leaves, rc, ra = _stage_oracle(st, torch.float32)
    (rc.sum() + ra.sum()).backward()
    for k in STAGE_NAMES:
        assert float(leaves[k].grad[0, torch.cat([culled, never])].abs().max()) == 0.0, k
        assert float(leaves[k].grad[0, wk["composited"]].abs().reshape(S.N_PLAIN, -1).amax(1).min()) > 0.0, k
    assert float(ra.detach()[0, 16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16].abs().max()) == 0.0


def _subsets(radii, wk):
    return {"all": (radii.reshape(-1) > 0).nonzero()[:, 0], "past the first batch": wk["late"].nonzero()[:, 0]}


def test_float32_oracle_meets_the_stage_bounds_on_the_deep_scene():
    """Widest kernel, two cameras, background: what test_stage_compositing_at_every_width asks of the HIP kernels."""
    st = S.stage_inputs("deep", 2, 32)
    wk = _walk(st)
    l64, rc64, ra64 = _stage_oracle(st, torch.float64)
    l32, rc32, ra32 = _stage_oracle(st, torch.float32)
    ok = agreeing_pixels(rc32, ra32, rc64, ra64)
    assert 1.0 - ok.double().mean().item() <= MAX_FLIPPED
    v, va = S.upstream(rc64.shape, ra64.shape, ok)
    want = S.oracle_grads(l64, (rc64, ra64), (v, va))
    got = S.oracle_grads(l32, (rc32, ra32), (v, va))
    rows = lambda d: S.flat_rows({k: d[k] for k in STAGE_NAMES})  # noqa: E731
    worst, counts, _ = compare_grads(rows(got), rows(want), _subsets(st["radii"], wk))
    assert not failing_subsets(counts), (counts, worst)
    for k in STAGE_NAMES:
        assert rel_inf(got[k].sum(1), want[k].sum(1)) < SUM_TOL, k
    assert rel_inf(got["backgrounds"], want["backgrounds"]) < POSE_GRAD_TOL
    assert float(want["backgrounds"].abs().min()) > 0.0


@pytest.mark.parametrize("name", ["c3-33ch", "c2-16ch-antialiased", "c3-sh-per-camera"])
def test_float32_oracle_meets_the_end_to_end_bounds_on_the_deep_scene(name):
    ins, Ks, kw = S.e2e_inputs(name)
    l64, r64, a64, meta = S.oracle_e2e(ins, Ks, kw)
    l32, r32, a32, _ = S.oracle_e2e(ins, Ks, kw, dtype=torch.float32)
    ok = agreeing_pixels(r32, a32, r64, a64)
    assert 1.0 - ok.double().mean().item() <= MAX_FLIPPED
    v, va = S.upstream(r64.shape, a64.shape, ok)
    want = S.oracle_grads(l64, (r64, a64), (v, va))
    got = S.oracle_grads(l32, (r32, a32), (v, va))
    C = ins["viewmats"].shape[0]
    for c in range(C):
        assert rel_inf(got["viewmats"][c, :3], want["viewmats"][c, :3]) < POSE_GRAD_TOL, c
        assert rel_inf(want["viewmats"][(c + 1) % C, :3], want["viewmats"][c, :3]) > 100 * POSE_GRAD_TOL  # swap: rejected
    assert rel_inf(got["backgrounds"], want["backgrounds"]) < POSE_GRAD_TOL
    seen = (meta["radii"] > 0).any(0).nonzero()[:, 0]
    shared = [k for k in S.E2E_NAMES if not (k == "colors" and S.E2E_CASES[name]["per_cam"])]  # the [N, ...] inputs
    worst, counts, _ = compare_grads({k: got[k] for k in shared}, {k: want[k] for k in shared}, {"all": seen})
    assert not failing_subsets(counts), (counts, worst)
    for k in shared:
        assert rel_inf(got[k].sum(0), want[k].sum(0)) < SUM_TOL, k
    if S.E2E_CASES[name]["per_cam"]:
        rows = (meta["radii"].reshape(-1) > 0).nonzero()[:, 0]
        worst, counts, _ = compare_grads(S.flat_rows({"colors": got["colors"]}), S.flat_rows({"colors": want["colors"]}),
                                         {"all": rows})
        assert not failing_subsets(counts), (counts, worst)
        assert float(want["colors"][:, :, (S.SH_DEGREE + 1) ** 2:].abs().max()) == 0.0  # the unused bands
