"""GPU: Localizer(mode="map") with MapConfig.merge_voxel -- a map with a resolution -- at 160x120, "ED", with the synthetic
room, the settings, the yardstick and the drift bound of tests/test_gpu_map_localizer.py.

(a) A voxel so small that nothing can share one: the 6-frame constant twist with merge_voxel = 1e-4 m.  Precondition,
    with the mirror on the final map of the run without the option (which holds every row any frame ever had): no two
    rows in one voxel.  Then merged is 0 at the reset and on every frame, and poses, steps and added rows are bit for
    bit those of the run without the option.
(b) A working resolution: s = the median nearest-neighbour distance of frame 0's cloud in the world (numpy, here),
    merge_voxel = FACTOR * s, on the 5 + 5 there-and-back.  No frame lost, rows merged at the reset, map_size below the
    unmerged run's at every frame, and the absolute error per frame under the bound of the map tests: twice the running
    sum of the yardstick's pair errors.
(c) Together with the other options: the same run with free_rho = 0.05 and evict = True in a capacity the merged map of
    (b) outgrows, its rows after the fourth frame (a frame is inserted before it is merged, so no capacity below
    W * H can hold the first one).  On two frames the map before the merge is copied, and what merge leaves -- rows,
    colours, stamps (the maxima of stamps that differ: every frame observes), survivors -- is the mirror's in every
    bit; rows are evicted on the way out; the map is never full; n_live is consistent after every call.
(d) The evaluation driver with map_merge_voxel on the way out: the report's merged_per_frame is the run's.

Measured on the MI355X (NOTES.md, "Map resolution"): s = 0.02833 m.  FACTOR: the bound holds at 1.0, the first of 1.0,
0.75, 0.5, with per-frame errors of 7.5e-4, 4.2e-4, 5.8e-4, 9.7e-4, 7.0e-4 m on the way out against bounds of 1.6e-3 ..
6.8e-3 and 1.8e-4 .. 9.9e-4 on the way back against 8.1e-3 .. 1.4e-2; the unmerged run: 7.9e-4, 3.6e-4, 4.0e-4, 5.9e-4,
4.1e-4, then 3.4e-5 .. 9.8e-4.  At 0.75 s and 0.5 s NOTHING shares a voxel on this sequence -- merged is 0 at the reset
and on every frame -- and the runs are the unmerged run bit for bit: the bound holds there as it does unmerged, and the
test would be (a) again.  At 1.0 s a merge removes 276 rows of frame 0's 19 200 and 25 .. 38 of the 126 .. 157 a frame
adds: a voxel of the cloud's own spacing rarely holds two of its points.  The frames on the way back, which add and
merge nothing, do not repeat bit for bit from run to run on the merged map (steps and the fourth digit of the error
differ; the map itself is the same bits every time), which the unmerged run does: from frame 6 on a fused row's scale
takes the largest cull radius from 1.99 to 2.02 px, past the 2 px up to which the render context uses its tiny-splat
backward, and the general backward sums with float atomics (NOTES.md).  Nothing here compares those frames between
runs; (a), (d) and the mirror checks use frames and quantities that repeat."""
import numpy as np
import pytest
import torch

from gsplatloc_amd.mapping import MapConfig
from gsplatloc_amd.synthetic import write_replica_constant_twist, write_replica_there_and_back
from tests import map_merge_ref as ref
from tests.test_gpu_map_localizer import N_B, N_OUT, H, W, _check_drift, _yardstick
from tests.test_gpu_map_view_localizer import _bits, _run

pytestmark = pytest.mark.gpu
N_C = 2 * N_OUT + 1
TINY = 1.0e-4  # (a): metres; the smallest side MapConfig takes is 9.54e-5
FACTOR = 1.0  # (b), (c): merge_voxel in units of s


def median_nn(points):
    """The median over the rows of the distance to the nearest other row (float64, brute force in blocks)."""
    p = np.asarray(points, dtype=np.float64)
    sq = (p * p).sum(axis=1)
    nearest = np.empty(len(p))
    for a in range(0, len(p), 1024):
        d2 = sq[a:a + 1024, None] + sq[None, :] - 2.0 * (p[a:a + 1024] @ p.T)
        d2[np.arange(d2.shape[0]), a + np.arange(d2.shape[0])] = np.inf
        nearest[a:a + 1024] = np.sqrt(np.maximum(d2.min(axis=1), 0.0))
    return float(np.median(nearest))


@pytest.fixture(scope="module")
def seq_b(tmp_path_factory):
    root = tmp_path_factory.mktemp("merge_seq_b")
    write_replica_constant_twist(root, W, H, N_B, rot_deg=0.4, trans=0.01)
    return root


@pytest.fixture(scope="module")
def there_and_back(tmp_path_factory):
    """The there-and-back files, the yardstick's pair errors, the run without the option, s, and the merged run."""
    root = tmp_path_factory.mktemp("merge_seq_c")
    write_replica_there_and_back(root, W, H, N_OUT, rot_deg=0.4, trans=0.01)
    plain = _run(root, N_C, MapConfig())
    s = median_nn(plain["before"][0])
    return dict(root=root, eT=_yardstick(root, N_C), plain=plain, s=s,
                merged=_run(root, N_C, MapConfig(merge_voxel=FACTOR * s)))


def test_a_voxel_nothing_can_share_changes_nothing(seq_b, capsys):
    plain = _run(seq_b, N_B, MapConfig())
    final = plain["loc"].map.points.cpu().numpy()
    assert len(final) == plain["results"][-1].map_size and ref.occupancy(final, TINY) == 1  # the precondition
    tiny = _run(seq_b, N_B, MapConfig(merge_voxel=TINY))
    (p1, s1, a1), (p2, s2, a2) = _bits(plain), _bits(tiny)
    with capsys.disabled():
        print(f"[merge] (a) largest pose difference {float((plain['traj'] - tiny['traj']).abs().max()):.3e}; steps "
              f"{s1} / {s2}, added {a1} / {a2}")
    assert tiny["loc"].merged_at_reset == 0 and [r.merged for r in tiny["results"]] == [0] * (N_B - 1)
    assert all(r.merged is None for r in plain["results"]) and plain["loc"].merged_at_reset is None
    assert not any(r.lost for r in tiny["results"])
    assert np.array_equal(p1, p2) and s1 == s2 and a1 == a2


def test_a_working_resolution(there_and_back, capsys):
    t = there_and_back
    plain, run = t["plain"], t["merged"]
    with capsys.disabled():
        print(f"[merge] (b) s = {t['s']:.5f} m, merge_voxel = {FACTOR} s")
        _check_drift("C map", plain, t["eT"])
        print(f"[merge] (b) merged at the reset {run['loc'].merged_at_reset}, per frame "
              f"{[r.merged for r in run['results']]}; map rows merged / unmerged "
              f"{[(a.map_size, b.map_size) for a, b in zip(run['results'], plain['results'])]}")
        _check_drift(f"C map merge {FACTOR} s", run, t["eT"])  # no frame lost, every frame under 2 sum eT_i
    assert run["loc"].merged_at_reset > 0 and run["after_reset"] == W * H - run["loc"].merged_at_reset
    assert all(a.map_size < b.map_size for a, b in zip(run["results"], plain["results"]))
    sizes = [run["after_reset"]] + [r.map_size for r in run["results"]]
    assert [b - a for a, b in zip(sizes, sizes[1:])] == [r.added - r.merged for r in run["results"]]
    assert sizes[-1] == run["loc"].map.n_live and not run["loc"].map.full


def test_the_evaluation_driver_reports_the_merges(there_and_back):
    from gsplatloc_amd.data import Parser
    from gsplatloc_amd.eval import evaluate_room
    from tests.test_gpu_map_localizer import ITERS

    t = there_and_back
    h, run = FACTOR * t["s"], t["merged"]
    parser = Parser("Replica", "room0", normalize=True, input_folder=str(t["root"]))
    r = evaluate_room(parser, ITERS, N_OUT, sequential=True, map_mode=True, map_merge_voxel=h)
    # the frames on the way out repeat bit for bit: the report is the run's
    assert r["merge_voxel"] == h and r["merge_every"] == 1 and r["lost_frames"] == 0 and r["map_full"] is False
    assert r["merged_at_reset"] == run["loc"].merged_at_reset
    assert r["merged_per_frame"] == [x.merged for x in run["results"][:N_OUT]] and sum(r["merged_per_frame"]) > 0
    assert r["map_gaussians"] == W * H - r["merged_at_reset"] + sum(r["added_per_frame"]) - sum(r["merged_per_frame"])
    sparse = evaluate_room(parser, ITERS, 4, sequential=True, map_mode=True, map_merge_voxel=h, map_merge_every=2)
    assert sparse["merged_per_frame"][0] == 0 and sparse["merged_per_frame"][2] == 0 and sparse["merged_per_frame"][1] > 0
    plain = evaluate_room(parser, ITERS, 2, sequential=True, map_mode=True)
    assert "merged_per_frame" not in plain and "merge_voxel" not in plain
    with pytest.raises(ValueError, match="map_merge_voxel"):
        evaluate_room(parser, ITERS, 2, sequential=True, map_merge_voxel=h)


CHECKED = (1, N_OUT)  # (c): the calls of track whose merge is held against the mirror


def run_with_the_other_options(root, config):
    """_run of tests/test_gpu_map_view_localizer.py with GaussianMap.merge wrapped: n_live around every call, and on
    the frames CHECKED a host copy of the map before the merge and of what it left."""
    from gsplatloc_amd.data import Parser
    from gsplatloc_amd.localizer import Localizer
    from gsplatloc_amd.my_gsplat import TrackerConfig
    from tests.test_gpu_map_localizer import ITERS

    parser = Parser("Replica", "room0", normalize=True, input_folder=str(root))
    depth, rgb, pose = parser.frame(0)
    loc = Localizer(parser.K, W, H, TrackerConfig(max_steps=ITERS), mode="map", map_config=config)
    m, merge, log, frame = loc.map, loc.map.merge, [], [0]

    def wrapped():
        n = m.n_live
        keep = frame[0] in CHECKED
        host = lambda a: a[:m.n_live].cpu().numpy().copy()  # noqa: E731
        before = (host(m.means), host(m.colors), host(m.stamps)) if keep else None
        out = merge()
        after = (host(m.means), host(m.colors), host(m.stamps), m.survivors.cpu().numpy().copy()) if keep else None
        log.append(dict(frame=frame[0], n=n, out=out, n_after=m.n_live, before=before, after=after))
        return out

    m.merge = wrapped
    loc.reset(depth, rgb, pose)
    sizes, results, gts, full = [m.n_live], [], [pose], []
    for i in range(1, N_C):
        depth, rgb, pose = parser.frame(i)
        frame[0] = i
        results.append(loc.track(depth, rgb, gt_c2w=pose))
        gts.append(pose)
        sizes.append(m.n_live)
        full.append(m.full)
    return dict(traj=loc.trajectory, gts=torch.stack(gts), results=results, loc=loc, log=log, sizes=sizes, full=full)


def check_the_merges(run, merge_voxel):
    """What every logged merge left is the mirror's, in every bit; n_live is consistent."""
    checked = 0
    for c in run["log"]:
        removed, kept = c["out"]
        assert removed + kept == c["n"] and c["n_after"] == kept
        if c["before"] is None:
            continue
        want = ref.merge(*c["before"], merge_voxel)
        assert (removed, kept) == (want["counters"][1], want["counters"][0])
        means, colors, stamps, survivors = c["after"]
        if removed > 0:
            assert np.array_equal(survivors, want["ids"])
        for got, name in ((means, "means"), (colors, "colors"), (stamps, "stamps")):
            assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), want[name].view(np.uint32)), (c["frame"], name)
        fused = want["k_of"] > 1
        assert fused.any() or removed == 0
        checked += 1
    return checked


def test_together_with_the_other_options(there_and_back, capsys):
    t = there_and_back
    h = FACTOR * t["s"]
    # a capacity the merged map of (b) outgrows: its rows after the fourth of the five frames on the way out.  It holds
    # a whole frame (a frame is inserted BEFORE it is merged, so the first one needs W * H rows), and the fifth frame
    # is short of room by about the rows it adds
    merged_sizes = [r.map_size for r in t["merged"]["results"]]
    cap = merged_sizes[N_OUT - 2]
    assert W * H <= cap < merged_sizes[N_OUT - 1], (cap, merged_sizes)
    run = run_with_the_other_options(t["root"], MapConfig(merge_voxel=h, free_rho=0.05, evict=True, capacity=cap))
    results = run["results"]
    with capsys.disabled():
        err = _check_drift(f"C map merge {FACTOR} s, free 0.05, evict at {cap}", run, t["eT"])
        print(f"[merge] (c) added {[r.added for r in results]}, evicted {[r.evicted for r in results]}, removed "
              f"{[r.removed for r in results]}, merged {[r.merged for r in results]}, map {run['sizes']}, error "
              f"{['%.3e' % e for e in err]}")
    assert not any(run["full"]) and not any(r.lost for r in results)
    assert all(n <= cap for n in run["sizes"]), run["sizes"]
    assert any(r.evicted > 0 for r in results[:N_OUT]), [r.evicted for r in results]
    assert run["loc"].map.frame_index == N_C - 1  # every frame observed: the stamps the merges take the maxima of
    sizes = run["sizes"]
    assert [b - a for a, b in zip(sizes, sizes[1:])] == [r.added - r.evicted - r.removed - r.merged for r in results]
    assert [r.map_size for r in results] == sizes[1:]
    assert len(run["log"]) == N_C and [c["out"][0] for c in run["log"][1:]] == [r.merged for r in results]
    assert check_the_merges(run, h) == len(CHECKED)
