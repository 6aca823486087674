"""CPU guard of tests/pose_ref.py: the far poses take the quaternion branches they are named after, the float32 run of
the reference loop stays as close to its float64 run as when the pose-step tests were written (their bounds are
multiples of that distance), and the loop's early-stop bookkeeping follows a scripted loss sequence."""
import pytest
import torch

from oracle import tracker_oracle as T
from tests.pose_ref import (FAR_CASES, PoseHyper, branch, far_poses, random_loss_sums, random_v_viewmats,
                            reference_pose_loop)
from tests.scenes import small_pose

# float32 run against float64 run over 25 steps, measured when this file was written (largest over the five poses)
FLOOR_Q, FLOOR_T, FLOOR_GRAD = 1.7e-7, 6.5e-7, 8e-7
STOP_LOSSES = (5.0, 4.0, 3.0, 2.5, 2.6, 2.4, 2.7, 2.8, 2.9, 1.0, 0.9, 0.8)


def test_every_far_pose_takes_its_branch():
    poses = far_poses()
    assert set(poses) == set(FAR_CASES)
    assert {b for _, _, b in FAR_CASES.values()} == {"c0", "c1", "c2", "c3"}
    for name, c2w in poses.items():
        R = c2w[:3, :3]
        assert torch.allclose(R @ R.T, torch.eye(3, dtype=torch.float64), atol=1e-14) and float(torch.det(R)) > 0.999
        for M in (R, R.float()):  # the device sees the float32 matrix
            assert branch(M) == FAR_CASES[name][2], (name, branch(M))
        # the restated conditions pick what the oracle picks: its quaternion reproduces R
        q = T.rotation_matrix_to_quaternion(R.contiguous())
        assert torch.allclose(T.quaternion_to_rotation_matrix(q), R, atol=1e-7), name
        assert abs(float(q.norm()) - 1.0) < 1e-7
        want = {"c0": 0, "c1": 1, "c2": 2, "c3": 3}[FAR_CASES[name][2]]
        if name != "trace>0":
            assert int(q.abs().argmax()) == want, (name, q)
    assert float(poses["pi_exact"][:3, :3].trace()) == -1.0
    assert branch(torch.eye(3)) == "c0"


@pytest.mark.parametrize("name", list(FAR_CASES))
def test_float32_reference_loop_stays_at_its_floor(name):
    init = far_poses()[name]
    gt = init @ small_pose(0.3, 0.01)
    n = 25
    vv, ls = random_v_viewmats(n, seed=11), random_loss_sums(n, seed=12, pixels=256)
    hp = PoseHyper()
    r64 = reference_pose_loop(torch.float64, init, gt, vv, ls, hp)
    r32 = reference_pose_loop(torch.float32, init, gt, vv, ls, hp)
    dq = max(float((a["q"] - b["q"]).abs().max()) for a, b in zip(r32, r64))
    dt = max(float((a["t"] - b["t"]).abs().max()) for a, b in zip(r32, r64))
    # the seven gradient entries of a step against the largest of them
    g7 = lambda r: torch.cat([r["grad_q"], r["grad_t"]])  # noqa: E731
    dg = max(float((g7(a) - g7(b)).abs().max() / g7(b).abs().max()) for a, b in zip(r32, r64))
    q0 = T.rotation_matrix_to_quaternion(init[:3, :3].contiguous())
    travel_q = float((r64[-1]["q"] - q0).norm())
    travel_t = float((r64[-1]["t"] - init[:3, 3]).norm())
    print(f"[floor] {name}: q {dq:.2e} (travelled {travel_q:.2e}), t {dt:.2e} (travelled {travel_t:.2e}), grad {dg:.2e}")
    assert dq <= 4 * FLOOR_Q and dt <= 4 * FLOOR_T and dg <= 4 * FLOOR_GRAD, (dq, dt, dg)
    # a wrong gradient term moves the pose by orders more than the floor
    assert travel_q > 1e3 * FLOOR_Q and travel_t > 1e3 * FLOOR_T, (travel_q, travel_t)
    assert r64[-1]["step"] == n and r64[-1]["stopped"] == 1 and r64[-2]["stopped"] == 0  # max_steps = 25


def _scripted(early_stop, max_steps, n_calls):
    init = far_poses()["m00"]
    hp = PoseHyper(min_step=2, patience=3, early_stop=early_stop, max_steps=max_steps, depth_w=1.0, edge_w=0.0)
    ls = torch.zeros(n_calls, 3, dtype=torch.float64)
    ls[:, 0] = torch.tensor(STOP_LOSSES[:n_calls], dtype=torch.float64) * hp.width * hp.height
    return reference_pose_loop(torch.float64, init, init @ small_pose(0.3, 0.01), random_v_viewmats(n_calls, 5), ls, hp)


def test_reference_loop_follows_the_scripted_early_stop():
    rec = _scripted(True, 100, 11)
    # step > min_step: index 2 does not update the best; 2.5 at 3, 2.4 at 5, then three worse losses stop the loop at 8
    want = [(-1, 0, 0), (-1, 0, 0), (-1, 0, 0), (3, 0, 0), (3, 1, 0), (5, 0, 0), (5, 1, 0), (5, 2, 0), (5, 3, 1),
            (5, 3, 1), (5, 3, 1)]
    assert [(r["best_step"], r["counter"], r["stopped"]) for r in rec] == want
    assert [r["step"] for r in rec] == [1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9]
    assert [float(r["best_loss"]) for r in rec[3:]] == [2.5, 2.5, 2.4, 2.4, 2.4, 2.4, 2.4, 2.4]
    assert float(rec[2]["best_loss"]) == float("inf")
    assert float(rec[8]["loss"]) == 2.9  # the stopping iteration still reports its loss ...
    for k in ("q", "t", "m", "v", "lr", "c2w", "viewmat"):  # ... and takes no optimiser step
        assert torch.equal(rec[8][k], rec[7][k]) and torch.equal(rec[10][k], rec[7][k]), k
        assert not torch.equal(rec[7][k], rec[6][k]), k
    # best errors are those of the pose the best loss was seen at (the pose BEFORE that iteration's step)
    assert float(rec[8]["best_eT"]) == float(rec[5]["eT"]) and float(rec[8]["best_eR"]) == float(rec[5]["eR"])


def test_reference_loop_takes_its_last_step_at_max_steps():
    rec = _scripted(False, 6, 8)
    assert [r["stopped"] for r in rec] == [0, 0, 0, 0, 0, 1, 1, 1]
    assert [r["step"] for r in rec] == [1, 2, 3, 4, 5, 6, 6, 6]
    assert all(r["best_step"] == -1 and r["counter"] == 0 for r in rec)  # no bookkeeping without early_stop
    for k in ("q", "t", "m", "v", "lr"):
        assert not torch.equal(rec[5][k], rec[4][k]), k  # iteration 5 took its step
        assert torch.equal(rec[7][k], rec[5][k]), k
    assert torch.equal(rec[5]["c2w"], rec[4]["c2w"]) and torch.equal(rec[7]["viewmat"], rec[4]["viewmat"])  # final pose
    hp = PoseHyper()
    assert abs(float(rec[5]["lr"][0]) - hp.quat_lr * hp.gamma ** 6) < 1e-18
