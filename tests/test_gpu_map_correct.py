"""GPU: gsl_map_correct (csrc/map_correct.hip) against the numpy mirror tests/map_correct_ref.py -- the means bit for bit,
both counters equal -- and GaussianMap.origins / correct / rows_up_to / loop_constraint on real kernels.

The rows: 1, 63, 64, 65 (on either side of a wave), 257 (a workgroup and a row), 19 200 (one 160 x 120 frame), 60 000
(235 workgroups and a tail) and 131 372 (more rows than one trip of the 512-workgroup grid), against tables of 1, 3 and
300 frames.  Origins non-decreasing as the map makes them, with rows in front of the table (-1) and behind it
(n_frames); tables that mix the identity (also with -0.0 for its zeros) with rotations up to 10 degrees and
translations up to 0.3 m; rows within 8 m, some NaN, inf and -0.0.  One wave that spans four origins.  Guard words
around the means, and the origins and the table, keep their bits.

The loop (tests/map_correct_ref.room_loop): eight frames of the box room at 160 x 120, the camera on a 10 cm circle
looking at a corner, the tracker's trajectory drifting by 0.3 degrees and 5 mm a frame -- 2.1 degrees and 3.2 cm at
frame 7.  Every frame is inserted whole at its DRIFTED pose.  Spreading the one constraint "frame 7 stood at its true
pose" brings the RMS distance of the rows from where the true poses put them to 0.018 of its value on the mirror; the
test asks for a half.  ``loop_constraint`` on the uncorrected map, against the rows of frame 0 alone, finds frame 7's
true pose from the drifted one: 6.1e-6 m and 1.8e-6 (Frobenius, rotation) on the mirror tests/map_align_ref.py; the
bound is twice the 1e-3 / 1e-3 that tests/test_gpu_map_align.py holds the same kernel to."""
import numpy as np
import pytest
import torch

from gsplatloc_amd import _lib
from gsplatloc_amd.mapping import GaussianMap, MapConfig, spread_correction
from gsplatloc_amd.synthetic import replica_intrinsics, room_depth
from tests import map_correct_ref as ref
from tests import map_evict_ref, map_free_ref, map_merge_ref
from tests import test_map_correct_cpu as cpu
from tests.test_abi import prototypes
from tests.test_map_refine_cpu import refine_args

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
ROWS = [1, 63, 64, 65, 257, 19200, 60000, 512 * 256 + 300]
FRAMES = [1, 3, 300]
GUARD = 8  # float32 words on either side of the means
FILL = 1.0e30


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _table(n_frames, rng):
    """float32 [n_frames,12]: every third entry the identity (every sixth with -0.0 for its zeros), the others a turn of
    up to 10 degrees and a shift of up to 0.3 m; a single frame gets a transform."""
    T = np.tile(np.eye(4), (n_frames, 1, 1))
    for k in range(n_frames):
        if n_frames == 1 or k % 3 != 1:
            T[k] = ref.twist(rng.uniform(0.0, 10.0), rng.uniform(0.0, 0.3), rng.normal(size=3), rng.normal(size=3))
    table = ref.table_of(T)
    for k in range(4, n_frames, 6):
        assert np.array_equal(table[k], ref.IDENTITY)
        table[k] = np.where(table[k] == 0, F32(-0.0), table[k])
    return table


def _case(n, n_frames, seed):
    rng = np.random.default_rng(seed)
    table = _table(n_frames, rng)
    origins = np.sort(rng.integers(0, n_frames, n)).astype(np.int32)
    means = rng.uniform(-8.0, 8.0, (n, 3)).astype(F32)
    if n >= 63:
        k = max(n // 50, 2)
        origins[:k] = -1  # in front of the table and behind it: still non-decreasing
        origins[-k:] = n_frames
        for j, value in enumerate((np.nan, np.inf, -np.inf, -0.0)):
            means[(k + 5 + 7 * np.arange(8) * (j + 1)) % n, j % 3] = value
        means[n // 2, :] = -0.0
    return means, origins, table


def _run(means, origins, table, fill=0x5A5A5A5A5A5A5A5A):
    """The entry point on means inside guard words.  Returns (means, counters); the guards, the origins and the table
    keep their bits."""
    lib, ptr, st = _lib.load_library(), _lib.ptr, _lib.current_stream()
    n = len(means)
    buf = torch.full((2 * GUARD + 3 * n,), FILL, device=DEV)
    inner = buf[GUARD:GUARD + 3 * n]
    inner.copy_(torch.from_numpy(means.reshape(-1)))
    o_t, t_t = torch.from_numpy(origins).to(DEV), torch.from_numpy(table).to(DEV)
    counters = torch.full((2,), fill, dtype=torch.int64, device=DEV)
    _lib.check(lib.gsl_map_correct(inner.data_ptr(), ptr(o_t), n, ptr(t_t), len(table), ptr(counters), st),
               "gsl_map_correct")
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + 3 * n:] == FILL).all())
    assert np.array_equal(o_t.cpu().numpy(), origins) and np.array_equal(_bits(t_t.cpu().numpy()), _bits(table))
    return inner.cpu().numpy().reshape(n, 3), tuple(counters.tolist())


def _check(means, origins, table, what):
    want = ref.correct(means, origins, table)
    got, counters = _run(means, origins, table)
    assert counters == want["counters"], (what, counters, want["counters"])
    assert np.array_equal(_bits(got), _bits(want["means"])), what
    return want


@pytest.mark.parametrize("n_frames", FRAMES)
@pytest.mark.parametrize("n", ROWS)
def test_correct_against_the_mirror(n, n_frames):
    means, origins, table = _case(n, n_frames, seed=n + n_frames)
    assert (np.diff(origins) >= 0).all()
    want = _check(means, origins, table, (n, n_frames))
    if n >= 63:  # every clause is in the case
        assert want["counters"][1] == 2 * max(n // 50, 2) and 0 < want["counters"][0] < n
        kept = ~want["moved"]
        assert np.array_equal(_bits(want["means"][kept]), _bits(means[kept]))
        assert not np.isfinite(means[kept & ~want["outside"]]).all() or n_frames > 1


def test_a_wave_that_spans_four_origins():
    rng = np.random.default_rng(11)
    table = np.stack([ref.table_of(ref.twist(2.0 + k, 0.05 * k, rng.normal(size=3), rng.normal(size=3))[None])[0]
                      for k in range(4)])
    table[2] = ref.IDENTITY
    for n, per in ((64, 16), (256, 16), (100, 7)):
        origins = np.minimum(np.arange(n) // per, 3).astype(np.int32) if n != 256 else (np.arange(n) // per % 4).astype(np.int32)
        means = rng.uniform(-8.0, 8.0, (n, 3)).astype(F32)
        want = _check(means, origins, table, (n, per))
        assert want["counters"] == (int((origins != 2).sum()), 0)


def test_no_rows_is_no_launch():
    lib = _lib.load_library()
    buf = torch.full((64,), FILL, device=DEV)
    counters = torch.full((2,), 77, dtype=torch.int64, device=DEV)
    origins = torch.zeros(4, dtype=torch.int32, device=DEV)
    assert lib.gsl_map_correct(buf.data_ptr(), origins.data_ptr(), 0, buf.data_ptr(), 3, counters.data_ptr(),
                               _lib.current_stream()) == 0
    torch.cuda.synchronize()
    assert counters.tolist() == [77, 77] and bool((buf == FILL).all())  # not even the zeroing launch


def test_bad_arguments_are_refused_without_a_launch(repo_root):
    """The refusals of tests/test_map_correct_cpu.py with device pointers: nothing is written."""
    lib = _lib.load_library()
    params = prototypes(repo_root)["gsl_map_correct"][1]
    buf = torch.full((4096,), 0x5A, dtype=torch.uint8, device=DEV)
    for what, over in cpu.REFUSED:
        assert lib.gsl_map_correct(*refine_args(params, dict(cpu.GOOD, **over), buf.data_ptr())) == cpu.BAD_ARG, what
    torch.cuda.synchronize()
    assert bool((buf == 0x5A).all())


# ---- GaussianMap on the device --------------------------------------------------------------------------------------
W, H = 160, 120
K = replica_intrinsics(W, H)
INTR = tuple(float(F32(a)) for a in (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))
NEAR, FAR = 0.01, 100.0


def _w2c(pose):
    return np.linalg.inv(np.asarray(pose, np.float64)).astype(F32)


def _prefixes_agree(m):
    o = m.origins[:m.n_live].cpu().numpy()
    return (np.diff(o) >= 0).all() and all(m.rows_up_to(f) == int((o <= f).sum()) for f in range(-1, int(o.max()) + 2))


def test_gaussian_map_carries_the_origins_and_corrects():
    true, _ = ref.room_loop()
    poses = [torch.from_numpy(p).float() for p in true]
    depths = [room_depth(W, H, K, p) for p in poses]
    rgb = torch.randint(0, 255, (H, W, 3), generator=torch.Generator().manual_seed(2)).float()
    cfg = MapConfig(origins=True, free_rho=0.05, evict=True, merge_voxel=0.05, capacity=3 * W * H)
    m = GaussianMap(W, H, cfg, DEV)
    assert m.origins.dtype == torch.int32 and m.origins.is_cuda and m.rows_up_to(5) == 0
    assert m.correct(np.tile(ref.twist(1.0, 0.1), (3, 1, 1))) == (0, 0)  # an empty map
    render, alphas = torch.full((H, W), 0.01), torch.ones(H, W)
    alphas[:, :8] = 0.25  # 8 H pixels are new per later frame
    assert m.insert_frame(depths[0], rgb, K, poses[0]) == (W * H, W * H)
    for k in (1, 2, 3):
        m.observe(depths[k], K, poses[k], NEAR, FAR)
        assert m.insert_frame(depths[k], rgb, K, poses[k], render, alphas, origin=2 * k) == (8 * H, 8 * H)
    n = m.n_live
    origins = np.array([0] * (W * H) + [2] * (8 * H) + [4] * (8 * H) + [6] * (8 * H), np.int32)
    assert np.array_equal(m.origins[:n].cpu().numpy(), origins) and _prefixes_agree(m)
    assert m.rows_up_to(0) == W * H and m.rows_up_to(3) == W * H + 8 * H and m.rows_up_to(6) == n
    with pytest.raises(ValueError, match="origin"):
        m.insert_frame(depths[0], rgb, K, poses[0], render, alphas, origin=5)
    # free space: a block of frame 0's rows and one of frame 4's, pulled to 60 % of their distance from the camera
    for lo, hi in ((1000, 1200), (W * H + 8 * H + 100, W * H + 8 * H + 300)):
        cam = torch.from_numpy(true[3][:3, 3]).float().to(DEV)
        m.means[lo:hi] = cam + (m.means[lo:hi] - cam) * 0.6
    means = m.points.cpu().numpy()
    kept = map_free_ref.select(means, _w2c(true[3]), INTR, depths[3].numpy(), F32(m._free_keep), 1, NEAR)["ids"]
    removed, stay = m.remove_seen_through(depths[3], K, poses[3], NEAR)
    assert removed == n - len(kept) >= 300 and np.array_equal(m.survivors.cpu().numpy(), kept)
    origins = origins[kept]
    assert np.array_equal(m.origins[:stay].cpu().numpy(), origins) and _prefixes_agree(m)
    # eviction: the least recently observed rows, wherever they came from (one more frame first, which looks the other
    # way: the rows that frame 3 has just stamped are then a frame old and may go)
    away = poses[3].clone()
    away[:3, :3] = away[:3, :3] @ torch.diag(torch.tensor([-1.0, 1.0, -1.0]))
    m.observe(room_depth(W, H, K, away), K, away, NEAR, FAR)
    stamps = m.stamps[:stay].cpu().numpy()
    assert int((stamps < m.frame_index).sum()) >= 5000
    kept = map_evict_ref.select(stamps, m.frame_index, cfg.evict_min_age, 5000)["ids"]
    evicted, stay = m.evict(5000)
    assert evicted == 5000 and np.array_equal(m.survivors.cpu().numpy(), kept)
    origins = origins[kept]
    assert np.array_equal(m.origins[:stay].cpu().numpy(), origins) and _prefixes_agree(m)
    # merge: a fused voxel keeps the origin of the row that stays
    kept = map_merge_ref.merge(m.points.cpu().numpy(), m.point_colors.cpu().numpy(), m.stamps[:stay].cpu().numpy(),
                               cfg.merge_voxel)["ids"]
    removed, stay = m.merge()
    assert removed > 1000 and np.array_equal(m.survivors.cpu().numpy(), kept)
    origins = origins[kept]
    assert np.array_equal(m.origins[:stay].cpu().numpy(), origins) and _prefixes_agree(m)
    assert sorted(set(origins.tolist())) == [0, 2, 4, 6]
    # correct: the mirror's rows bit for bit; frame 0 stays (the identity), frames 5 and 6 lie outside the transforms
    D = np.stack([np.eye(4)] + [ref.twist(0.5 * k, 0.01 * k) for k in range(1, 5)])
    means, ptr = m.points.cpu().numpy(), m.means.data_ptr()
    want = ref.correct(means, origins, ref.table_of(D))
    m._view_rows = stay
    assert m.correct(D) == want["counters"] == (int(np.isin(origins, (2, 4)).sum()), int((origins == 6).sum()))
    assert np.array_equal(_bits(m.points.cpu().numpy()), _bits(want["means"]))
    assert m.means.data_ptr() == ptr and m._view_rows == -1
    assert np.array_equal(m.origins[:stay].cpu().numpy(), origins)
    # ... and all-identity transforms change nothing
    assert m.correct(np.tile(np.eye(4), (9, 1, 1))) == (0, 0)
    assert np.array_equal(_bits(m.points.cpu().numpy()), _bits(want["means"]))


# ---- end to end: a drifting loop, closed --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loop():
    """(map with the eight frames inserted at their drifted poses, true poses, drifted poses, depth images, where the
    true poses put every row [n,3] float64)."""
    true, est = ref.room_loop()
    m = GaussianMap(W, H, MapConfig(origins=True, capacity=8 * W * H), DEV)
    rgb = torch.full((H, W, 3), 100.0)
    depths = [room_depth(W, H, K, torch.from_numpy(p).float()) for p in true]
    for k in range(8):
        assert m.insert_frame(depths[k], rgb, K, torch.from_numpy(est[k]).float())[1] == W * H
    rows, o = m.points.cpu().numpy().astype(np.float64), m.origins[:m.n_live].cpu().numpy()
    assert np.array_equal(o, np.repeat(np.arange(8), W * H))
    move = true @ np.linalg.inv(est)  # per frame: from where the drifted pose put a row to where the true one does
    truth = np.einsum("nij,nj->ni", move[o, :3, :3], rows) + move[o, :3, 3]
    return m, true, est, depths, truth


def test_loop_constraint_finds_the_true_pose_from_the_old_rows(loop):
    m, true, est, depths, _ = loop
    before = m.points.clone()
    c = m.loop_constraint(depths[7], K, torch.from_numpy(est[7]).float(), 0, NEAR)
    assert c.rows == m.rows_up_to(0) == W * H and c.alignment.moved and c.alignment.status == "CONVERGED"
    got = c.alignment.c2w.cpu().numpy().astype(np.float64)
    err_t, err_r = np.linalg.norm(got[:3, 3] - true[7][:3, 3]), np.sqrt(((got[:3, :3] - true[7][:3, :3]) ** 2).sum())
    was_t, was_r = np.linalg.norm(est[7][:3, 3] - true[7][:3, 3]), np.sqrt(((est[7][:3, :3] - true[7][:3, :3]) ** 2).sum())
    print(f"[correct] loop_constraint: {was_t:.3e} m / {was_r:.3e} -> {err_t:.3e} m / {err_r:.3e}; scores "
          f"{c.scores.tolist()} -> {c.aligned_scores.tolist()}")
    assert err_t < was_t and err_r < was_r
    assert err_t < 2e-3 and err_r < 2e-3  # twice what tests/test_gpu_map_align.py holds the same kernel to
    # the aligned pose agrees with more of the prefix, and only the prefix was judged
    assert c.aligned_scores[1] > c.scores[1] and c.scores[0] <= W * H and c.aligned_scores[0] <= W * H
    assert torch.equal(m.points, before)  # nothing in the map is written


def test_closing_the_loop_brings_the_rows_back(loop):
    m, true, est, depths, truth = loop
    rows = m.points.cpu().numpy()
    o = m.origins[:m.n_live].cpu().numpy()
    D = spread_correction(est, 0, 7, true[7] @ np.linalg.inv(est[7]))
    want = ref.correct(rows, o, ref.table_of(D))
    assert m.correct(D) == want["counters"] == (7 * W * H, 0)
    after = m.points.cpu().numpy()
    assert np.array_equal(_bits(after), _bits(want["means"])) and np.array_equal(_bits(after[:W * H]), _bits(rows[:W * H]))
    e0, e1 = ref.rms(rows - truth), ref.rms(after - truth)
    print(f"[correct] room loop of 8: RMS {e0:.4f} m -> {e1:.4f} m, x {e1 / e0:.3f}")
    assert e1 / e0 <= 0.5


# ---- Localizer(mode="map") and the evaluation driver on the device ------------------------------------------------------
N_SEQ, ITERS = 6, 2000


@pytest.fixture(scope="module")
def seq(tmp_path_factory):
    from gsplatloc_amd.synthetic import write_replica_constant_twist

    root = tmp_path_factory.mktemp("correct_seq")
    write_replica_constant_twist(root, W, H, N_SEQ, rot_deg=0.4, trans=0.01)
    return root


def test_the_localizer_closes_a_loop_on_the_device(seq):
    from tests.test_gpu_map_view_localizer import _run

    run = _run(seq, N_SEQ, MapConfig(origins=True))
    loc, last = run["loc"], N_SEQ - 1
    added = [r.added for r in run["results"]]
    n, o = loc.map.n_live, loc.map.origins[:loc.map.n_live].cpu().numpy()
    assert not any(r.lost for r in run["results"]) and all(a > 0 for a in added)
    assert np.array_equal(o, np.repeat(np.arange(N_SEQ), [run["after_reset"]] + added))
    # the last frame's ground truth as the constraint
    old, rows = loc.trajectory.cpu().double().numpy(), loc.map.points.cpu().numpy()
    gt = run["gts"][last].cpu()
    out = loc.close_loop(0, last, gt)
    D = spread_correction(old, 0, last, gt.double().numpy() @ np.linalg.inv(old[last]))
    new = loc.trajectory.cpu().double().numpy()
    assert np.array_equal(new[0], old[0]) and np.abs(new[last] - gt.double().numpy()).max() <= 1e-6
    assert np.abs(new - D @ old).max() <= 1e-6
    assert out.moved == n - run["after_reset"] and out.outside == 0 and out.frames == last
    after = loc.map.points.cpu().numpy()
    assert np.array_equal(_bits(after[:run["after_reset"]]), _bits(rows[:run["after_reset"]]))
    want = ref.correct(rows, o, ref.table_of(new @ np.linalg.inv(old)))["means"].astype(np.float64)
    assert np.abs(after - want).max() <= 1e-5  # the table itself is the localizer's: new old^-1 from its float32 poses
    assert abs(out.max_trans - np.linalg.norm(D[:, :3, 3], axis=1).max()) <= 1e-6


def test_the_evaluation_driver_reports_the_origins(seq):
    from gsplatloc_amd.data import Parser
    from gsplatloc_amd.eval import evaluate_room

    parser = Parser("Replica", "room0", normalize=True, input_folder=str(seq))
    r = evaluate_room(parser, ITERS, None, sequential=True, map_mode=True, map_origins=True)
    assert r["origins"] is True and r["origins_non_decreasing"] is True and r["frames"] == N_SEQ - 1
    assert len(r["rows_per_origin"]) == N_SEQ and sum(r["rows_per_origin"]) == r["map_gaussians"]
    assert r["rows_per_origin"][0] == W * H and r["rows_per_origin"][1:] == r["added_per_frame"]
    plain = evaluate_room(parser, ITERS, None, sequential=True, map_mode=True)
    assert "origins" not in plain and "rows_per_origin" not in plain
