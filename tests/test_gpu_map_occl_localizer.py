"""GPU: Localizer(mode="map") with MapConfig.view_occlusion_rho -- every frame tracked against the rows in view that no
nearer surface of the map hides -- at 160x120, "ED", with the settings, the yardstick and the drift bound of
tests/test_gpu_map_localizer.py and the runner of tests/test_gpu_map_view_localizer.py.

(a) Neutral in a room seen from inside: on the 16-frame sweep of the view test (1 degree, 1 cm per frame, guard 8 px) the
    mirror culls nothing (tests/test_map_occl_cpu.py asserts it for the ground-truth poses; here view_culled == 0 at
    every frame), so the run with occlusion must equal the run with view_guard_px alone bit for bit (poses, steps, added
    rows) if two runs of the latter repeat bit for bit in this process, and otherwise lie within their difference.
(b) A camera that passes a panel (write_replica_passing_panel: 0.8 x 0.6 m at z = 1, 2 cm per frame along x, 24 frames
    centred on x = 0, no rotation).  With ground-truth poses and frame 0's points the mirror culls 1176 of 18 360 rows in
    the band at the last pose, 6.4 % (asserted: at least 5 %).  No frame is lost; the per-frame absolute error stays
    within twice the running sum of the yardstick's pair errors; tracked + view_culled is the mirror's count of rows in
    the band at every start pose, and both are the mirror's; view_culled > 0 from some frame on; the rows added in total
    are at most 1.5 x those of the run with view_guard_px alone (a culled row that is re-inserted would show up here: the
    wall behind the panel is 6 % of the band, and it would come back every frame).
Measured on the MI355X: (a) the guard alone repeats bit for bit and the run with occlusion gives the same bits, 0 rows
culled on every frame; (b) tracks with the constant-velocity start as it is, no rotation added; errors 5.2e-3 .. 1.5e-2 m
under bounds of 1.3e-2 .. 2.9e-1; culled 0, 56, 0, 0, 183, 112, 122, 305, ... 1 305, every frame from the fifth on; rows
added 5 031, with the guard alone 6 506."""
import numpy as np
import pytest

from gsplatloc_amd.mapping import MapConfig
from gsplatloc_amd.synthetic import write_replica_constant_twist, write_replica_passing_panel
from tests import map_occl_ref as ref
from tests.test_gpu_map_localizer import H, W, _check_drift, _check_growth, _yardstick
from tests.test_gpu_map_view_localizer import GUARD, N_SWEEP, SWEEP_DEG, SWEEP_TRANS, _bits, _run

pytestmark = pytest.mark.gpu
N_PASS, RHO, CELL, WINDOW = 24, 0.05, 4, 1


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    root = tmp_path_factory.mktemp("occl_sweep")
    write_replica_constant_twist(root, W, H, N_SWEEP, rot_deg=SWEEP_DEG, trans=SWEEP_TRANS)
    return root


@pytest.fixture(scope="module")
def passing(tmp_path_factory):
    """The files, the ground-truth poses, the yardstick's pair errors and the run with the guard alone."""
    root = tmp_path_factory.mktemp("occl_pass")
    poses = write_replica_passing_panel(root, W, H, N_PASS)
    return dict(root=root, poses=poses, eT=_yardstick(root, N_PASS),
                guard=_run(root, N_PASS, MapConfig(view_guard_px=GUARD)))


def test_neutral_in_a_room_seen_from_inside(sweep, capsys):
    first, second = (_run(sweep, N_SWEEP, MapConfig(view_guard_px=GUARD)) for _ in range(2))
    culled = _run(sweep, N_SWEEP, MapConfig(view_guard_px=GUARD, view_occlusion_rho=RHO))
    (p1, s1, a1), (p2, s2, a2), (pc, sc, ac) = _bits(first), _bits(second), _bits(culled)
    repeats = np.array_equal(p1, p2) and s1 == s2 and a1 == a2
    d_pose = float((first["traj"] - second["traj"]).abs().max())
    d_steps, d_added = max(abs(a - b) for a, b in zip(s1, s2)), max(abs(a - b) for a, b in zip(a1, a2))
    c_pose = float((first["traj"] - culled["traj"]).abs().max())
    c_steps, c_added = max(abs(a - b) for a, b in zip(s1, sc)), max(abs(a - b) for a, b in zip(a1, ac))
    with capsys.disabled():
        print(f"[occl] (a) guard alone twice: repeats bit for bit {repeats}; largest difference pose {d_pose:.3e}, "
              f"steps {d_steps}, added {d_added}; with occlusion against the first: pose {c_pose:.3e}, steps {c_steps}, "
              f"added {c_added}; culled {[r.view_culled for r in culled['results']]}")
    assert all(r.view_culled is None for r in first["results"])
    assert [r.view_culled for r in culled["results"]] == [0] * (N_SWEEP - 1)
    assert not any(r.lost for r in culled["results"])
    if repeats:
        assert np.array_equal(pc, p1) and sc == s1 and ac == a1
    else:
        assert c_pose <= d_pose and c_steps <= d_steps and c_added <= d_added


def test_the_panel_hides_a_part_of_the_band(passing):
    """The sequence is what the bounds assume: with ground-truth poses and frame 0's points the mirror culls at least
    5 % of the rows in the band at the last pose, and none at the first."""
    run = passing["guard"]
    pts0 = run["before"][0]
    assert pts0.shape == (W * H, 3)
    share = []
    for p in passing["poses"]:
        r = ref.select(pts0, ref.w2c_of(p.numpy()), run["intr"], W, H, GUARD, run["near"], run["far"], CELL, WINDOW, RHO)
        share.append(r["counters"][3] / int(r["band"].sum()))
    print("[occl] share of frame 0's rows in the band that are culled, per pose", ["%.3f" % s for s in share])
    assert share[0] == 0.0 and share[-1] >= 0.05


def test_the_guard_alone_holds_on_the_passing_camera(passing, capsys):
    """The sequence is not too hard for the tracker: the local map without the option loses no frame and stays in its
    bounds on it (otherwise a failure below would say nothing about the occlusion rule)."""
    with capsys.disabled():
        _check_drift("pass guard alone", passing["guard"], passing["eT"])
    _check_growth(passing["guard"])


def test_passing_camera_tracked_against_the_visible_rows(passing, capsys):
    run = _run(passing["root"], N_PASS, MapConfig(view_guard_px=GUARD, view_occlusion_rho=RHO))
    with capsys.disabled():
        _check_drift("pass occlusion", run, passing["eT"])  # no frame lost, every frame under 2 sum eT_i
        print(f"[occl] pass: tracked {[r.tracked for r in run['results']]}, culled "
              f"{[r.view_culled for r in run['results']]}, violations {[r.view_violations for r in run['results']]}")
    _check_growth(run)
    for k, (r, prefix) in enumerate(zip(run["results"], run["before"])):
        want = ref.select(prefix, ref.w2c_of(r.init_c2w.cpu().numpy()), run["intr"], W, H, GUARD, run["near"],
                          run["far"], CELL, WINDOW, RHO)
        assert r.tracked + r.view_culled == int(want["band"].sum()), (k, r.tracked, r.view_culled)
        assert (r.tracked, r.view_culled) == (want["counters"][0], want["counters"][3]), (k, want["counters"])
    # from some frame on every frame culls: by the middle of the sequence the panel's edge has moved 12 px over the
    # wall (80 px focal length, 2 cm a frame, depths 1 m and 3 m: 1.07 px a frame), three cells of 4 px
    culled = [r.view_culled for r in run["results"]]
    first_cull = max([k + 1 for k, c in enumerate(culled) if c == 0], default=0)  # the frame after the last one without
    assert first_cull <= N_PASS // 2 and all(c > 0 for c in culled[first_cull:]), culled
    added, alone = sum(r.added for r in run["results"]), sum(r.added for r in passing["guard"]["results"])
    with capsys.disabled():
        print(f"[occl] pass: rows added {added}, with the guard alone {alone}; map rows {run['results'][-1].map_size} / "
              f"{passing['guard']['results'][-1].map_size}; first frame with a culled row {first_cull + 1}")
    assert added <= 1.5 * alone, (added, alone)
