"""``mapping.optimise_pose_graph``: least squares over a pose graph on SE(3), float64, on the host.

The cases are those of tests/test_map_correct_cpu.py: the drifting circle (cameras evenly on a circle of radius 0.5 m,
the tracker adding the same body-frame error to every motion, 200 rows per frame written at the drifted poses) with the
one constraint "the last frame stood at its true pose relative to the first", which ``spread_correction`` closes to
0.18 .. 0.19 of the rows' RMS error and which has to fall to a half or less here as there; a consistent graph (true
odometry, drifted start), which has to come back to the truth; and two laps of the circle with three overlapping
constraints, which closed one after the other by ``spread_correction`` undo each other -- the first two are left
violated by 4.7e-2 and 5.1e-2 (rad and m) -- and which the graph satisfies together.

Measured with this implementation: the consistent graph 1.9e-15 from the truth in 4 iterations; the circles 0.212,
0.210 and 0.208; the two laps' three residuals at most 4.6e-7, the rows at 0.026 m against 0.091 m sequentially
(0.29 x) and 0.344 m before."""
import numpy as np
import pytest
import torch

from gsplatloc_amd.mapping import (PoseGraphResult, _se3_exp, _se3_log, optimise_pose_graph, spread_correction)
from tests import map_correct_ref as ref
from tests.test_map_correct_cpu import CIRCLES, circle_rows

inv = np.linalg.inv


def odometry(poses):
    return [inv(poses[k]) @ poses[k + 1] for k in range(len(poses) - 1)]


def moved_rows(rows, origins, new, old):
    """Where the rows land when every frame's rows follow its pose: D_k = new_k old_k^-1, in float64."""
    D = np.asarray(new) @ inv(np.asarray(old))
    return np.einsum("nij,nj->ni", D[origins, :3, :3], np.asarray(rows, np.float64)) + D[origins, :3, 3]


def residual(Z, Ti, Tj):
    return float(np.linalg.norm(np.concatenate(_se3_log(inv(Z) @ inv(Ti) @ Tj))))


def cost_of(poses, odo, loops, weights=None):
    edges = [(k, k + 1, Z, 1.0 if weights is None else weights[k]) for k, Z in enumerate(odo)] + list(loops)
    return sum(w * residual(Z, poses[i], poses[j]) ** 2 for i, j, Z, w in edges)


def two_laps():
    """(true, drifted, the three constraints): 48 frames, twice round the circle of 24, 0.3 degrees and 5 mm a frame."""
    true = np.concatenate([ref.circle_poses(24, 0.5)] * 2)
    return true, ref.drifted(true, 0.3, 0.005), [(0, 24), (10, 34), (20, 47)]


def test_a_consistent_graph_comes_back_to_the_truth():
    true = ref.circle_poses(48, 0.5)
    start = ref.drifted(true, 0.3, 0.005)
    r = optimise_pose_graph(start, odometry(true), [(0, 47, inv(true[0]) @ true[47], 1e4)], 0)
    err = np.abs(r.poses - true).max()
    print(f"[pose graph] consistent graph of 48: {err:.2e} from the truth in {r.iterations} iterations, cost "
          f"{r.cost_before:.3e} -> {r.cost_after:.3e}")
    assert isinstance(r, PoseGraphResult) and r.poses.dtype == np.float64 and r.poses.shape == (48, 4, 4)
    assert err <= 1e-9 and r.iterations <= 10 and r.converged
    assert r.cost_after <= 1e-20 < r.cost_before and r.loop_residuals.shape == (1,) and r.loop_residuals[0] <= 1e-9


@pytest.mark.parametrize("n,rot_deg,trans", CIRCLES)
@pytest.mark.parametrize("by", ["index", "path"])
def test_the_drifting_circle(n, rot_deg, trans, by):
    est, true, rows, want, origins = circle_rows(n, rot_deg, trans)
    r = optimise_pose_graph(est, odometry(est), [(0, n - 1, inv(true[0]) @ true[n - 1], 1e4)], 0, by=by)
    before, after = ref.rms(rows - want), ref.rms(moved_rows(rows, origins, r.poses, est) - want)
    D = spread_correction(est, 0, n - 1, true[-1] @ inv(est[-1]), by)
    spread = ref.rms(moved_rows(rows, origins, D @ est, est) - want)
    print(f"[pose graph] circle of {n}, {rot_deg} deg / {trans * 1e3:g} mm a frame, by {by}: RMS {before:.4f} m -> "
          f"{after:.4f} m, x {after / before:.3f} (spread_correction: x {spread / before:.3f}); {r.iterations} iterations, "
          f"edge residual {r.loop_residuals[0]:.2e}")
    assert r.converged and after / before <= 0.5
    assert np.array_equal(r.poses[0], est[0]) and r.loop_residuals[0] <= 1e-5
    assert r.cost_after < 1e-3 * r.cost_before


def test_three_overlapping_constraints_hold_together():
    true, est, cons = two_laps()
    loops = [(i, j, inv(true[i]) @ true[j], 1e4) for i, j in cons]
    r = optimise_pose_graph(est, odometry(est), loops, 0)
    # the same constraints closed one after the other, each spread over its own span
    cur = est.copy()
    for i, j in cons:
        target = cur[i] @ inv(true[i]) @ true[j]
        cur = spread_correction(cur, i, j, target @ inv(cur[j]), "index") @ cur
    sequential = [residual(inv(true[i]) @ true[j], cur[i], cur[j]) for i, j in cons]
    rng = np.random.default_rng(0)
    z = rng.uniform(1.0, 3.0, (48, 200, 1))
    cam = np.concatenate([rng.uniform(-0.5, 0.5, (48, 200, 2)) * z, z, np.ones((48, 200, 1))], -1)
    rows = np.einsum("kij,knj->kni", est, cam)[..., :3].reshape(-1, 3)
    want = np.einsum("kij,knj->kni", true, cam)[..., :3].reshape(-1, 3)
    origins = np.repeat(np.arange(48), 200)
    e0 = ref.rms(rows - want)
    e_seq, e_graph = (ref.rms(moved_rows(rows, origins, p, est) - want) for p in (cur, r.poses))
    print(f"[pose graph] two laps, three constraints: residuals sequentially {['%.2e' % v for v in sequential]}, by the "
          f"graph {['%.2e' % v for v in r.loop_residuals]}; rows RMS {e0:.4f} m -> {e_seq:.4f} m sequentially, "
          f"{e_graph:.4f} m by the graph (x {e_graph / e_seq:.2f}); {r.iterations} iterations")
    assert r.converged and r.loop_residuals.shape == (3,) and (r.loop_residuals <= 1e-5).all()
    assert [residual(Z, r.poses[i], r.poses[j]) for i, j, Z, _ in loops] == pytest.approx(r.loop_residuals.tolist(), abs=1e-12)
    assert e_graph <= 0.5 * e_seq
    assert max(sequential[:2]) > 1e-2  # what the graph is for: the later closures undo the earlier ones


def test_held_nodes_keep_every_bit():
    true, est, cons = two_laps()
    est = est.astype(np.float32).astype(np.float64)
    est[3, 0, 3], est[5, 1, 3] = -0.0, -0.0  # a sign that an arithmetic round trip would lose
    est[2, 2, 3] = np.float64(np.float32(0.1))
    loops = [(i, j, inv(true[i]) @ true[j], 1e4) for i, j in cons[1:]]  # the smallest anchor is 10
    r = optimise_pose_graph(torch.from_numpy(est), odometry(est), loops, 10)
    assert np.array_equal(r.poses[:11], est[:11]) and np.array_equal(np.signbit(r.poses[:11]), np.signbit(est[:11]))
    assert not np.array_equal(r.poses[11], est[11]) and (r.loop_residuals <= 1e-5).all()
    # every node held: nothing to do, the poses come back as they are
    r = optimise_pose_graph(est, odometry(est), loops, 47)
    assert np.array_equal(r.poses, est) and np.array_equal(np.signbit(r.poses), np.signbit(est))
    assert r.iterations == 0 and r.converged and r.cost_after == r.cost_before > 0


@pytest.mark.parametrize("by", ["index", "path"])
def test_the_cost_is_stationary_at_the_solution(by):
    """A central-difference gradient of the cost itself, in the right perturbation of every free node."""
    est, true, *_ = circle_rows(24, 0.5, 0.010)
    est[5] = est[4] @ ref.twist(0.5, 0.0005)  # one short step: "path" weighs it up
    odo = odometry(est)
    loops = [(0, 23, inv(true[0]) @ true[23], 1e4), (3, 17, inv(true[3]) @ true[17] @ ref.twist(0.2, 0.004), 50.0)]
    r = optimise_pose_graph(est, odo, loops, 2, by=by)
    weights = None
    if by == "path":
        steps = np.array([np.linalg.norm(Z[:3, 3]) for Z in odo])
        weights = steps.mean() / np.maximum(steps, 0.01 * steps.mean())
        assert weights.max() > 5.0
    assert cost_of(est, odo, loops, weights) == pytest.approx(r.cost_before, rel=1e-12)
    assert cost_of(r.poses, odo, loops, weights) == pytest.approx(r.cost_after, rel=1e-9)
    h, worst = 1e-6, 0.0
    for k in range(3, 24):
        for a in range(6):
            d = np.zeros(6)
            d[a] = h
            up, down = r.poses.copy(), r.poses.copy()
            up[k] = r.poses[k] @ _se3_exp(d[:3], d[3:])
            down[k] = r.poses[k] @ _se3_exp(-d[:3], -d[3:])
            worst = max(worst, abs(cost_of(up, odo, loops, weights) - cost_of(down, odo, loops, weights)) / (2 * h))
    print(f"[pose graph] by {by}: cost {r.cost_before:.3e} -> {r.cost_after:.3e}, largest gradient entry {worst:.2e}")
    assert r.converged and r.cost_after < r.cost_before and worst <= 1e-6 * r.cost_before
    assert np.array_equal(r.poses[:3], est[:3])


def test_the_graph_commutes_with_a_change_of_the_world_frame():
    true, est, cons = two_laps()
    loops = [(i, j, inv(true[i]) @ true[j], 1e4) for i, j in cons]
    G = ref.twist(40.0, 3.0, (1.0, -2.0, 0.5), (0.2, 0.9, -0.4))
    a = optimise_pose_graph(est, odometry(est), loops, 0, by="path")
    b = optimise_pose_graph(G @ est, odometry(G @ est), loops, 0, by="path")
    assert np.abs(b.poses - G @ a.poses).max() <= 1e-9
    assert b.loop_residuals == pytest.approx(a.loop_residuals.tolist(), abs=1e-9)


def test_the_dense_and_the_sparse_solve_agree():
    pytest.importorskip("scipy.sparse")
    true, est, cons = two_laps()
    loops = [(i, j, inv(true[i]) @ true[j], 1e4) for i, j in cons]
    for by in ("index", "path"):
        dense = optimise_pose_graph(est, odometry(est), loops, 0, by=by, solver="dense")
        sparse = optimise_pose_graph(est, odometry(est), loops, 0, by=by, solver="sparse")
        default = optimise_pose_graph(est, odometry(est), loops, 0, by=by)
        assert np.abs(dense.poses - sparse.poses).max() <= 1e-9
        assert np.array_equal(default.poses, sparse.poses)  # scipy imports here: the default is the sparse solve
        assert dense.converged and sparse.converged


def test_without_scipy_the_solve_is_dense(monkeypatch):
    import builtins

    true, est, cons = two_laps()
    loops = [(i, j, inv(true[i]) @ true[j], 1e4) for i, j in cons]
    dense = optimise_pose_graph(est, odometry(est), loops, 0, solver="dense")
    real = builtins.__import__

    def no_scipy(name, *a, **k):
        if name.split(".")[0] == "scipy":
            raise ImportError(name)
        return real(name, *a, **k)

    monkeypatch.setattr(builtins, "__import__", no_scipy)
    r = optimise_pose_graph(est, odometry(est), loops, 0)
    assert np.array_equal(r.poses, dense.poses)


def test_levenberg_takes_over_where_the_full_step_would_raise_the_cost():
    """A start far from the minimum: 48 nodes whose drift has reached 34 degrees, pulled round by one edge."""
    true = ref.circle_poses(48, 0.5)
    est = ref.drifted(true, 0.7, 0.02)
    r = optimise_pose_graph(est, odometry(est), [(0, 47, inv(true[0]) @ true[47], 1e4)], 0, iters=60)
    assert r.converged and r.cost_after < 1e-2 * r.cost_before and r.loop_residuals[0] <= 1e-5
    short = optimise_pose_graph(est, odometry(est), [(0, 47, inv(true[0]) @ true[47], 1e4)], 0, iters=1)
    assert short.iterations == 1 and not short.converged and short.cost_after < short.cost_before


def test_what_is_refused():
    true, est, cons = two_laps()
    odo, Z = odometry(est), inv(true[0]) @ true[24]
    as_it_is = inv(est[0]) @ est[24]  # the edge the start satisfies: its residual is what is multiplied on
    good = dict(poses=est, odometry=odo, loops=[(0, 24, Z, 1e4)], fixed_upto=0, by="index")
    optimise_pose_graph(**good)
    optimise_pose_graph(**dict(good, loops=[]))  # no loop edge: the odometry is satisfied as it is
    quarter, skew, nan = ref.twist(90.0, 0.0), Z.copy(), Z.copy()
    skew[0, 0] += 1e-3
    nan[1, 3] = np.nan
    bad_poses = est.copy()
    bad_poses[7, 0, 3] = np.inf
    for what, over in (("a residual of 90 degrees", dict(loops=[(0, 24, as_it_is @ quarter, 1e4)])),
                       ("an odometry edge 120 degrees off", dict(odometry=odo[:5] + [odo[5] @ ref.twist(120.0, 0.0)] + odo[6:])),
                       ("i out of range", dict(loops=[(-1, 24, Z, 1e4)])), ("j out of range", dict(loops=[(0, 48, Z, 1e4)])),
                       ("i == j", dict(loops=[(24, 24, Z, 1e4)])), ("i > j", dict(loops=[(24, 0, Z, 1e4)])),
                       ("an index that is no integer", dict(loops=[(0.0, 24, Z, 1e4)])),
                       ("a Z that is not rigid", dict(loops=[(0, 24, skew, 1e4)])),
                       ("a Z with a NaN", dict(loops=[(0, 24, nan, 1e4)])), ("a Z of another shape", dict(loops=[(0, 24, Z[:3], 1e4)])),
                       ("a weight of 0", dict(loops=[(0, 24, Z, 0.0)])), ("a NaN weight", dict(loops=[(0, 24, Z, float("nan"))])),
                       ("an edge without a weight", dict(loops=[(0, 24, Z)])),
                       ("a pose that is not finite", dict(poses=bad_poses)), ("poses of another shape", dict(poses=est[:, :3])),
                       ("too few odometry edges", dict(odometry=odo[:-1])), ("an odometry edge that is not rigid", dict(odometry=[skew] + odo[1:])),
                       ("fixed_upto < 0", dict(fixed_upto=-1)), ("fixed_upto >= n", dict(fixed_upto=48)),
                       ("fixed_upto no integer", dict(fixed_upto=1.0)), ("by", dict(by="time")),
                       ("iters", dict(iters=0)), ("tol", dict(tol=-1.0)), ("solver", dict(solver="qr"))):
        try:
            optimise_pose_graph(**dict(good, **over))
        except ValueError:
            continue
        raise AssertionError(f"{what}: not refused")
    assert optimise_pose_graph(**dict(good, loops=[(0, 24, as_it_is @ ref.twist(80.0, 0.0), 1.0)])).poses.shape == (48, 4, 4)
