"""GPU: Localizer(mode="map") with MapConfig.evict -- a map that lives in its capacity -- at 160x120, "ED", with the
settings, the yardstick and the drift bound of tests/test_gpu_map_localizer.py.

(a) Neutral with room to spare: the 6-frame constant twist of that file with evict=True and the default capacity,
    against two runs without it, by the rule of tests/test_gpu_map_view_localizer.py: bit-identical if the uncut mode
    repeats itself, else within its own difference.  Nothing is evicted.
(b) The sweep of tests/test_gpu_map_view_localizer.py (16 frames, 1 degree and 1 cm per frame) in a map whose capacity is
    the uncut run's map_size after frame N_SWEEP // 2, taken from that run here.  Precondition, with the mirror on the
    ground-truth poses and the uncut run's rows: before every later frame the rows that frame does not observe are at
    least as many as the rows it adds (its need when the map is at its capacity) -- otherwise the run could only pass
    by dropping rows.  Without the option the run at that capacity ends full, with added < selected on some frame.
    With it: never full, map_size <= capacity on every frame, evicted > 0 on some frame, no frame lost, and the drift
    bound of the uncut mode (twice the running sum of the yardstick's pair errors), which the uncut run holds too.
(c) The same with view_guard_px = 8, and tracked <= map_size - added.
(d) The evaluation driver with map_evict on the sweep: the report's evicted_per_frame is the run's.

Measured on the MI355X (NOTES.md, "Bounded map"): (a) repeats bit for bit, nothing evicted; (b) capacity 22 544, rows not
observed before frames 9 .. 15: 3 051 .. 5 145 against needs of 404 .. 438; evicted 0 x 8, then 404, 438, 409, 435, 409,
436, 410, each frame what it adds; final error 7.027e-3 m against 7.032e-3 m uncut; (c) the same evictions, 7.022e-3 m."""
import numpy as np
import pytest
import torch

from gsplatloc_amd.mapping import MapConfig
from gsplatloc_amd.synthetic import write_replica_constant_twist
from tests import map_evict_ref as ref
from tests.test_gpu_map_localizer import ITERS, N_B, H, W, _check_drift, _yardstick
from tests.test_gpu_map_view_localizer import N_SWEEP, SWEEP_DEG, SWEEP_TRANS, _bits, _run

pytestmark = pytest.mark.gpu
CUT = N_SWEEP // 2  # the capacity is the uncut map after this frame


@pytest.fixture(scope="module")
def seq_b(tmp_path_factory):
    root = tmp_path_factory.mktemp("evict_seq_b")
    write_replica_constant_twist(root, W, H, N_B, rot_deg=0.4, trans=0.01)
    return root


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    """The sweep's files, its ground-truth poses, the yardstick's pair errors, the uncut map-mode run and the capacity."""
    root = tmp_path_factory.mktemp("evict_sweep")
    poses = write_replica_constant_twist(root, W, H, N_SWEEP, rot_deg=SWEEP_DEG, trans=SWEEP_TRANS)
    uncut = _run(root, N_SWEEP, MapConfig())
    return dict(root=root, poses=poses, eT=_yardstick(root, N_SWEEP), uncut=uncut,
                capacity=uncut["results"][CUT - 1].map_size)


def test_neutral_with_room_to_spare(seq_b, capsys):
    first, second = _run(seq_b, N_B, MapConfig()), _run(seq_b, N_B, MapConfig())
    bounded = _run(seq_b, N_B, MapConfig(evict=True))
    (p1, s1, a1), (p2, s2, a2), (pc, sc, ac) = _bits(first), _bits(second), _bits(bounded)
    repeats = np.array_equal(p1, p2) and s1 == s2 and a1 == a2
    d_pose = float((first["traj"] - second["traj"]).abs().max())
    d_steps, d_added = max(abs(a - b) for a, b in zip(s1, s2)), max(abs(a - b) for a, b in zip(a1, a2))
    c_pose = float((first["traj"] - bounded["traj"]).abs().max())
    c_steps, c_added = max(abs(a - b) for a, b in zip(s1, sc)), max(abs(a - b) for a, b in zip(a1, ac))
    with capsys.disabled():
        print(f"[evict] (a) uncut twice: repeats bit for bit {repeats}; largest difference pose {d_pose:.3e}, steps "
              f"{d_steps}, added {d_added}; evict=True against the first uncut run: pose {c_pose:.3e}, steps {c_steps}, "
              f"added {c_added}")
    assert all(r.evicted == 0 and not r.lost for r in bounded["results"]) and not bounded["loc"].map.full
    assert all(r.evicted is None for r in first["results"])
    assert bounded["loc"].map.frame_index == N_B - 1 and first["loc"].map.frame_index == 0
    if repeats:
        assert np.array_equal(pc, p1) and sc == s1 and ac == a1
    else:
        assert c_pose <= d_pose and c_steps <= d_steps and c_added <= d_added


def test_the_sweep_leaves_enough_rows_unobserved(sweep, capsys):
    """The precondition of (b) and (c), and that the uncut mode holds its bound on this sequence."""
    from gsplatloc_amd.data import Parser

    run, cap = sweep["uncut"], sweep["capacity"]
    with capsys.disabled():
        _check_drift("sweep uncut", run, sweep["eT"])
    parser = Parser("Replica", "room0", normalize=True, input_folder=str(sweep["root"]))
    cfg = MapConfig()
    assert W * H < cap < run["results"][-1].map_size  # the map outgrows it
    table = []
    for k in range(CUT + 1, N_SWEEP):  # frame k, tracked from the rows before[k - 1]
        depth = parser.frame(k)[0].cpu().numpy()
        rows = run["before"][k - 1]
        seen = ref.observed(rows, ref.w2c_of(sweep["poses"][k].numpy()), run["intr"], depth, ref.keep_of(cfg.depth_rho),
                            cfg.observe_window_px, cfg.view_reach_px, run["near"], run["far"])
        need = run["results"][k - 1].added
        table.append((k, len(rows), int((~seen).sum()), need))
    with capsys.disabled():
        print(f"[evict] capacity {cap}; (frame, uncut rows before it, of them not observed at its pose, rows it adds) "
              f"{table}")
    assert all(unseen >= need for _, _, unseen, need in table), table
    assert any(need > 0 for _, _, _, need in table), table


def _check_bounded(tag, sweep, config, capsys):
    cap = sweep["capacity"]
    run = _run(sweep["root"], N_SWEEP, config)
    results = run["results"]
    with capsys.disabled():
        err = _check_drift(tag, run, sweep["eT"])  # no frame lost, every frame under 2 sum eT_i
        uncut = (sweep["uncut"]["traj"][:, :3, 3] - sweep["uncut"]["gts"][:, :3, 3]).norm(dim=1).tolist()
        print(f"[evict] {tag}: abs error per frame, bounded / uncut "
              f"{[('%.3e' % a, '%.3e' % b) for a, b in zip(err, uncut)]}")
        print(f"[evict] {tag}: capacity {cap}, evicted {[r.evicted for r in results]}, added "
              f"{[r.added for r in results]}, map {[r.map_size for r in results]}")
    assert not run["loc"].map.full and not any(r.lost for r in results)
    assert all(r.map_size <= cap for r in results), [r.map_size for r in results]
    assert any(r.evicted > 0 for r in results), [r.evicted for r in results]
    sizes = [run["after_reset"]] + [r.map_size for r in results]
    assert [b - a for a, b in zip(sizes, sizes[1:])] == [r.added - r.evicted for r in results]
    assert sizes[-1] == run["loc"].map.n_live
    # a frame evicts only what it is short of: afterwards the map is exactly at its capacity
    assert all(r.map_size == cap for r in results if r.evicted > 0)
    return run


def test_without_the_option_the_map_fills_up(sweep):
    run = _run(sweep["root"], N_SWEEP, MapConfig(capacity=sweep["capacity"]))
    # ``full`` is set by the frame that appended fewer rows than it selected (GaussianMap.insert_frame): the rest of
    # that frame was dropped, and from then on the map is at its capacity and takes nothing in
    assert run["loc"].map.full and run["results"][-1].map_size == sweep["capacity"]
    assert sum(r.added for r in run["results"]) == sweep["capacity"] - W * H
    assert sum(r.added for r in run["results"]) < sum(r.added for r in sweep["uncut"]["results"])
    assert run["results"][-1].added == 0 and all(r.evicted is None for r in run["results"])


def test_the_evaluation_driver_reports_the_evictions(sweep):
    from gsplatloc_amd.data import Parser
    from gsplatloc_amd.eval import evaluate_room

    cap = sweep["capacity"]
    parser = Parser("Replica", "room0", normalize=True, input_folder=str(sweep["root"]))
    r = evaluate_room(parser, ITERS, N_SWEEP - 1, sequential=True, map_mode=True, map_capacity=cap, map_evict=True)
    assert r["evict"] is True and r["map_full"] is False and r["lost_frames"] == 0 and r["map_gaussians"] == cap
    assert len(r["evicted_per_frame"]) == N_SWEEP - 1 and sum(r["evicted_per_frame"]) > 0
    assert cap == W * H + sum(r["added_per_frame"]) - sum(r["evicted_per_frame"])
    plain = evaluate_room(parser, ITERS, 3, sequential=True, map_mode=True)
    assert "evicted_per_frame" not in plain and "evict" not in plain


def test_the_sweep_in_a_bounded_map(sweep, capsys):
    _check_bounded("sweep bounded", sweep, MapConfig(capacity=sweep["capacity"], evict=True), capsys)


def test_the_sweep_in_a_bounded_map_tracked_against_the_view(sweep, capsys):
    run = _check_bounded("sweep bounded guard 8", sweep,
                         MapConfig(capacity=sweep["capacity"], evict=True, view_guard_px=8.0), capsys)
    assert all(r.tracked <= r.map_size - r.added for r in run["results"])
