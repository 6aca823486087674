"""CPU guard of tests/loss_ref.py: the arbitrary-rows reference reproduces the project's own loss definitions in float64
(whole image: PoseTracker.tracking_loss and the oracle's tracking_loss; 16-aligned strips: parallel.strip_tracking_loss),
its shares add up, and the comparator the GPU tests import rejects three seeded defects of the kind a loss kernel can
have -- at every shape and strip of tests/test_gpu_loss_kernels.py where the defect changes the result at all."""
import pytest
import torch

import gsplatloc_amd.my_gsplat as M
from gsplatloc_amd.parallel import strip_tracking_loss
from gsplatloc_amd.synthetic import replica_intrinsics
from oracle import tracker_oracle as T
from tests import loss_ref as R

ATOL = 1e-12


def _autograd(fn, depth):
    d = depth.double().clone().requires_grad_()
    total, dl, sl = fn(d[None, ..., None])
    total.backward()
    return float(total.detach()), float(dl.detach()), float(sl.detach()), d.grad


@pytest.mark.parametrize("W,H", [(75, 52), (33, 18), (3, 3), (1, 1)])
@pytest.mark.parametrize("normal", [False, True])
def test_whole_image_reference_is_the_trackers_loss(W, H, normal):
    depth, target = R.loss_inputs(W, H, near_target=normal)
    g4 = target.double()[None, ..., None]
    lam_d, lam_n = (R.NORMAL_LAMBDA_DEPTH, R.NORMAL_LAMBDA) if normal else (R.LAMBDA_DEPTH, 0.0)
    K = replica_intrinsics(W, H, dtype=torch.float64)
    ref = R.evaluate(depth, target, 0, H, lam_d, 1 - lam_d - lam_n, lam_n)
    trk = M.PoseTracker(M.TrackerConfig(depth_lambda=lam_d, normal_lambda=lam_n))
    for name, fn in (("PoseTracker", lambda d: trk.tracking_loss(d, g4, K)),
                     ("oracle", lambda d: T.tracking_loss(d, g4, lam_d, lam_n, K))):
        total, dl, sl, grad = _autograd(fn, depth)
        assert abs(ref.total - total) <= ATOL, (name, ref.total, total)
        assert abs(ref.depth_sum / (W * H) - dl) <= ATOL and abs(ref.edge_sum / (W * H) - sl) <= ATOL, name
        assert float((ref.grad - grad).abs().max()) <= ATOL, name


@pytest.mark.parametrize("W,H", [(75, 52), (33, 18)])
@pytest.mark.parametrize("normal", [False, True])
def test_aligned_strips_are_strip_tracking_loss(W, H, normal):
    depth, target = R.loss_inputs(W, H, near_target=normal)
    g4 = target.double()[None, ..., None]
    lam_d, lam_n = (R.NORMAL_LAMBDA_DEPTH, R.NORMAL_LAMBDA) if normal else (R.LAMBDA_DEPTH, 0.0)
    K = replica_intrinsics(W, H, dtype=torch.float64)
    th = R.tile_rows(H)
    worst = 0.0
    for t0 in range(th):
        for t1 in range(t0 + 1, th + 1):
            r0, r1 = R.rows_of(t0, t1, H)
            ref = R.evaluate(depth, target, r0, r1, lam_d, 1 - lam_d - lam_n, lam_n)
            total, dl, sl, grad = _autograd(lambda d: strip_tracking_loss(d, g4, (t0, t1), H, lam_d, lam_n, K=K), depth)
            errs = (abs(ref.total - total), abs(ref.depth_sum / (W * H) - dl), abs(ref.edge_sum / (W * H) - sl),
                    float((ref.grad - grad).abs().max()))
            worst = max(worst, *errs)
            assert max(errs) <= ATOL, ((t0, t1), errs)
            # nothing outside the owned rows and their one-row halo receives a gradient
            assert float(ref.grad[:max(r0 - 1, 0)].abs().sum()) == 0.0 and float(ref.grad[r1 + 1:].abs().sum()) == 0.0
    print(f"[loss_ref] {W}x{H} normal={normal}: largest difference to strip_tracking_loss {worst:.1e}")


@pytest.mark.parametrize("normal", [False, True])
def test_shares_of_arbitrary_rows_add_up(normal):
    W, H = 75, 52
    depth, target = R.loss_inputs(W, H, near_target=normal)
    lam_d, lam_n = (R.NORMAL_LAMBDA_DEPTH, R.NORMAL_LAMBDA) if normal else (R.LAMBDA_DEPTH, 0.0)
    whole = R.evaluate(depth, target, 0, H, lam_d, 1 - lam_d - lam_n, lam_n)
    cuts = [0, 5, 23, 24, 51, 52]
    parts = [R.evaluate(depth, target, a, b, lam_d, 1 - lam_d - lam_n, lam_n) for a, b in zip(cuts[:-1], cuts[1:])]
    assert abs(sum(p.total for p in parts) - whole.total) <= ATOL
    assert abs(sum(p.depth_sum for p in parts) - whole.depth_sum) <= 1e-9  # sums of ~3900 terms of order 1
    assert abs(sum(p.edge_sum for p in parts) - whole.edge_sum) <= 1e-9
    assert float((sum(p.grad for p in parts) - whole.grad).abs().max()) <= ATOL
    empty = R.evaluate(depth, target, 7, 7, lam_d, 1 - lam_d - lam_n, lam_n)
    assert empty.total == 0.0 and float(empty.grad.abs().max()) == 0.0


def _gpu_cases():
    """(label, W, H, r0, r1, normal) of every launch tests/test_gpu_loss_kernels.py compares with the reference."""
    cases = [(f"whole {W}x{H}", W, H, 0, H, False) for W, H in R.WHOLE_SHAPES]
    for W, H in R.STRIP_SHAPES:
        cases += [(f"strip {W}x{H} rows {r0}:{r1}", W, H, r0, r1, False) for r0, r1 in R.strips_of(W, H)]
    cases += [(f"normal whole {W}x{H}", W, H, 0, H, True) for W, H in R.NORMAL_SHAPES]
    for W, H in R.NORMAL_STRIP_SHAPES:
        cases += [(f"normal strip {W}x{H} rows {r0}:{r1}", W, H, r0, r1, True) for r0, r1 in R.first_rest(H)]
    return cases


def _changes_the_result(defect, W, H, r0, r1):
    """Where the seeded defect is a different function at all (reasoned, not measured)."""
    if defect == "zero_pad":
        # every strip owns border pixels; a 1x1 image has a zero Sobel under either padding (the centre tap is 0)
        return (W, H) != (1, 1)
    return (r0, r1) != (0, H)  # a whole image has no halo rows and its own pixel count IS W*H


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_comparator_rejects_the_seeded_defect(defect):
    n_rejected = 0
    for label, W, H, r0, r1, normal in _gpu_cases():
        depth, target = R.loss_inputs(W, H, near_target=normal)
        lam_d, lam_n = (R.NORMAL_LAMBDA_DEPTH, R.NORMAL_LAMBDA) if normal else (R.LAMBDA_DEPTH, 0.0)
        args = (depth, target, r0, r1, lam_d, 1 - lam_d - lam_n, lam_n)
        sound, broken = R.evaluate(*args), R.evaluate(*args, defect=defect)
        R.assert_loss_close(sound, sound, normal, label)
        if _changes_the_result(defect, W, H, r0, r1):
            with pytest.raises(AssertionError):
                R.assert_loss_close(broken, sound, normal, label)
            n_rejected += 1
        else:
            assert torch.equal(broken.grad, sound.grad) and broken.total == sound.total, label
            assert (broken.depth_sum, broken.edge_sum) == (sound.depth_sum, sound.edge_sum), label
    assert n_rejected >= 20, n_rejected


def test_inputs_sit_on_no_sign_tie():
    """The guard every GPU case runs first, on all of them with the seed they use: float32 torch against float64 torch."""
    worst = {False: 0.0, True: 0.0}
    for label, W, H, r0, r1, normal in _gpu_cases():
        depth, target = R.loss_inputs(W, H, near_target=normal)
        lam_d, lam_n = (R.NORMAL_LAMBDA_DEPTH, R.NORMAL_LAMBDA) if normal else (R.LAMBDA_DEPTH, 0.0)
        worst[normal] = max(worst[normal], R.assert_no_sign_tie(depth, target, r0, r1, lam_d, 1 - lam_d - lam_n, lam_n,
                                                                label=label))
    print(f"[loss_ref] float32 against float64 gradient: tracking term {worst[False]:.1e}, "
          f"with the normal term {worst[True]:.1e}")
