"""GPU: gsl_map_pose_align_batch (csrc/map_align_batch.hip), bit for bit, against three things at once: the numpy mirror
(tests/map_align_batch_ref.py, which is tests/map_align_ref.py per pose and the three-valued done word on top), a single
gsl_map_pose_align call on each pose alone, and -- for a pose that was closed -- gsl_map_pose_info at the pose's final
float32 working copy, whose 30 integers the batch must have left in that pose's sums.

The scenes are those of tests/test_gpu_map_align.py: the corner view at 160x120 (the map is the back-projection of one
frame, the query 1 cm / 0.5 degrees away) and the single plane at 33x17.  The start poses of a batch are taken in turn
from six: the map's own pose (two steps, then CONVERGED), the query's true pose (CONVERGED at iteration 0), three poses
2, 3 and 6.4 cm off (three to five steps) and one that looks away from the room (FEW).  With a step bound of 3 cm the
last two of those three are TOO_FAR instead, so that one batch of two iterations holds STEPPED, CONVERGED, FEW and TOO_FAR
side by side, a pose that converges at iteration 0 next to one that never does; SINGULAR is the plane without damping;
and with three iterations the map's own pose converges on the last one and is left open (done = 1).  One thing varies at a
time around 5 poses, 8 iterations, damping 1e-3 and all 19 200 rows: the poses (1, 2, 5, 16) with the iterations (1, 2,
8), the damping (0), the rows (1 and 7 on either side of the fewest a step takes, 63 / 64 / 65 around a wave) and the
image (4x4).  Permuted poses give permuted results, two calls the same bits, the inputs and the guard words around every
buffer keep theirs, and a bad pose count or a null pointer is refused with nothing written."""
import ctypes

import numpy as np
import pytest
import torch

from gsplatloc_amd import _lib
from gsplatloc_amd.mapping import ALIGN_BATCH_MAX_POSES, GaussianMap, MapConfig
from gsplatloc_amd.synthetic import replica_intrinsics, room_depth
from tests import map_align_batch_ref as bref
from tests import map_align_ref as ref
from tests import map_info_ref as info
from tests import test_map_info_cpu as tinfo
from tests.test_gpu_map_align import FILL, GUARD, _guarded, _rows, _run
from tests.test_map_align_cpu import AT_MAP, BEYOND, DEFAULTS, KAPPA, KEEP, NEAR, QUERIES, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
BAD_ARG = -1
TRUTH = QUERIES["1cm0.5deg"]
STARTS = [AT_MAP, TRUTH, tinfo.yaw_pose((0.65, 0.1, 0.76), 38.0), tinfo.yaw_pose((0.6, 0.1, 0.8), 215.0),
          tinfo.yaw_pose((0.62, 0.1, 0.78), 36.5), tinfo.yaw_pose((0.63, 0.1, 0.77), 37.0)]
AT, EXACT, FAR, AWAY, NEARER, MIDDLE = range(6)


def _starts(n, first=0):
    """n start poses [n,4,4] float32 world-to-camera: STARTS in turn from ``first`` on, each round of six shifted by
    another millimetre along x so that no two poses of a batch are the same."""
    out = []
    for i in range(n):
        c2w = STARTS[(first + i) % 6].copy()
        c2w[0, 3] += 1e-3 * (i // 6)
        out.append(info.w2c_of(c2w))
    return np.stack(out)


def _call(lib, m_t, n, w_t, k, intr, d_t, w, h, a, sums, work, state, history):
    return lib.gsl_map_pose_align_batch(
        _lib.ptr(m_t), n, _lib.ptr(w_t), k, *(float(v) for v in intr), _lib.ptr(d_t), w, h, float(KEEP), float(BEYOND),
        float(KAPPA), float(NEAR), a["max_steps"], a["damping"], a["min_used"], a["max_rot"], a["max_trans"], a["eps_rot"],
        a["eps_trans"], sums, work, state, history, _lib.current_stream())


def _run_batch(means, w2cs, intr, depth, **over):
    """The entry point on buffers inside guard words; the inputs and the guards keep their bits.  Returns per pose what
    tests/map_align_batch_ref.pose_align_batch returns."""
    a = dict(DEFAULTS, **over)
    lib = _lib.load_library()
    (h, w), steps, k = depth.shape, a["max_steps"], len(w2cs)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)  # noqa: E731
    start = np.asarray(w2cs, F32).reshape(k, 16)
    m_t, w_t, d_t = t(means), t(start), t(depth)
    bufs = [_guarded(words) for words in (k * info.VALUES, k * 8, k * 14, k * steps * 10)]
    sums, work, state, history = (b[1] for b in bufs)
    _lib.check(_call(lib, m_t, means.shape[0], w_t, k, intr, d_t, w, h, a, sums.data_ptr(), work.data_ptr(),
                     state.data_ptr(), history.data_ptr()), "gsl_map_pose_align_batch")
    torch.cuda.synchronize()
    for buf, inner in bufs:
        assert bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + inner.numel():] == FILL).all())
    for dev, host in ((m_t, means), (w_t, start), (d_t, depth)):  # the inputs are only read
        assert np.array_equal(dev.cpu().numpy().view(np.uint32), np.ascontiguousarray(host).view(np.uint32))
    sums, work = sums.cpu().numpy().reshape(k, info.VALUES), work.cpu().numpy().view(F32).reshape(k, 4, 4)
    state, history = state.cpu().numpy().reshape(k, 14), history.cpu().numpy().reshape(k, steps, 10)
    return [(state[p, :12].view(np.float64).reshape(3, 4).copy(), work[p].copy(), int(state[p, 12]), int(state[p, 13]),
             history[p, :, :4].copy(), history[p, :, 4:].copy().view(np.float64), sums[p].copy()) for p in range(k)]


def _pose_info(means, work, intr, depth):
    """gsl_map_pose_info at the float32 pose ``work`` [4,4]: int64 [30]."""
    lib, ptr = _lib.load_library(), _lib.ptr
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)  # noqa: E731
    m_t, w_t, d_t = t(means), t(work.reshape(16)), t(depth)
    out = torch.full((info.VALUES,), FILL, dtype=torch.int64, device=DEV)
    h, w = depth.shape
    _lib.check(lib.gsl_map_pose_info(ptr(m_t), len(means), ptr(w_t), *(float(v) for v in intr), ptr(d_t), w, h, float(KEEP),
                                     float(BEYOND), float(KAPPA), float(NEAR), ptr(out), _lib.current_stream()),
               "gsl_map_pose_info")
    return out.cpu().numpy()


NAMES = ("pose", "working copy", "steps_taken", "done", "history integers", "history xi", "sums")


def _same(got, want, skip=()):
    for name, g, w in zip(NAMES, got, want):
        if name in skip:
            continue
        if isinstance(w, np.ndarray):
            assert same_bits(g, w), (name, g, w)
        else:
            assert g == w, (name, g, w)


def _check(means, w2cs, intr, depth, **over):
    """One batch against the mirror, against a single call per pose and, where closed, against gsl_map_pose_info.
    Returns (what the device left, the mirror's) per pose."""
    a = dict(DEFAULTS, **over)
    got = _run_batch(means, w2cs, intr, depth, **over)
    want = bref.pose_align_batch(means, w2cs, intr, depth, KEEP, BEYOND, KAPPA, NEAR, a["max_steps"], a["damping"],
                                 a["min_used"], a["max_rot"], a["max_trans"], a["eps_rot"], a["eps_trans"])
    assert len(got) == len(want) == len(w2cs)
    for p, (g, m) in enumerate(zip(got, want)):
        _same(g, m)  # state, work, every history row, done in 0 .. 2, and the sums the call leaves
        alone = _run(means, w2cs[p], intr, depth, **over)
        _same(g, alone, skip=("done", "sums"))
        assert alone[3] == (g[3] != 0)  # the single call's done is 0 or 1
        if g[3] == 2:
            assert np.array_equal(g[6], _pose_info(means, g[1], intr, depth)), p
    return got, want


@pytest.fixture(scope="module")
def corner():
    K = replica_intrinsics(160, 120)
    intr = tinfo.intrinsics(K)
    d_map = room_depth(160, 120, K, torch.from_numpy(AT_MAP).float()).numpy()
    return intr, tinfo.back_projection(d_map, intr, AT_MAP), room_depth(160, 120, K, torch.from_numpy(TRUTH).float()).numpy()


@pytest.mark.parametrize("steps", [1, 2, 8])
@pytest.mark.parametrize("n_poses", [1, 2, 5, 16])
def test_the_poses_and_the_iterations(n_poses, steps, corner):
    intr, means, depth = corner
    got, _ = _check(means, _starts(n_poses), intr, depth, max_steps=steps)
    assert got[0][4].shape == (steps, 4)
    if n_poses == 16 and steps == 8:  # every kind of pose is there, and each has finished and was closed
        assert {g[4][-1, 0] for g in got} == {ref.CONVERGED, ref.FEW} and all(g[3] == 2 for g in got)
        # the steps applied: FEW none, the true pose its one, and the poses finish at six different iterations
        assert [g[2] for g in got[:6]] == [3, 1, 6, 0, 4, 5] and sorted({g[2] for g in got}) == [0, 1, 2, 3, 4, 5, 6]


@pytest.mark.parametrize("n_poses", [1, 2, 5, 16])
def test_without_damping(n_poses, corner):
    intr, means, depth = corner
    _check(means, _starts(n_poses), intr, depth, damping=0.0)


@pytest.mark.parametrize("n", [1, 7, 63, 64, 65, 19200])
def test_the_rows(n, corner):
    intr, means, depth = corner
    some = _rows(means, n)
    assert some.shape == (n, 3)
    got, _ = _check(some, _starts(5), intr, depth)
    if n < 7:
        assert all((g[4][:, 0] == ref.FEW).all() and g[3] == 2 for g in got)
    if n == 7:
        assert got[AT][4][0, 0] == ref.STEPPED and got[AT][4][0, 1] == 7  # all seven used: solved


def test_a_four_by_four_image():
    K = replica_intrinsics(4, 4)
    intr = tinfo.intrinsics(K)
    d_map = room_depth(4, 4, K, torch.from_numpy(AT_MAP).float()).numpy()
    depth = room_depth(4, 4, K, torch.from_numpy(TRUTH).float()).numpy()
    got, _ = _check(tinfo.back_projection(d_map, intr, AT_MAP), _starts(2), intr, depth)
    for g in got:  # its inner pixels are one 2x2 block: too few rows, closed at once
        assert (g[4][:, 0] == ref.FEW).all() and 0 < g[4][0, 2] <= 4 and g[3] == 2


def test_four_statuses_side_by_side(corner):
    """Two iterations and a step bound of 3 cm: the map's pose steps twice and is still running, the true pose converges
    at iteration 0 and is closed at iteration 1, the pose that looks away has no rows, the pose 6.4 cm off is refused."""
    intr, means, depth = corner
    w2cs = _starts(4)
    got, _ = _check(means, w2cs, intr, depth, max_steps=2, max_trans=0.03)
    assert [g[4][:, 0].tolist() for g in got] == [[ref.STEPPED] * 2, [ref.CONVERGED] * 2, [ref.TOO_FAR] * 2, [ref.FEW] * 2]
    assert [g[3] for g in got] == [0, 2, 2, 2] and [g[2] for g in got] == [2, 1, 0, 0]
    for p in (FAR, AWAY):  # not moved: the pose keeps its bits
        assert same_bits(got[p][1], w2cs[p]) and same_bits(got[p][0], w2cs[p][:3].astype(np.float64))
    assert np.linalg.norm(got[FAR][5][0, 3:]) > 0.03 and not got[FAR][5][1].any()  # the refused step is on record once
    assert got[AWAY][6][28] == 0 and got[EXACT][6][28] > 18000


def test_a_pose_that_converges_on_the_last_iteration_stays_open(corner):
    intr, means, depth = corner
    got, want = _check(means, _starts(3), intr, depth, max_steps=3)
    assert [g[4][:, 0].tolist() for g in got] == [[ref.STEPPED, ref.STEPPED, ref.CONVERGED], [ref.CONVERGED] * 3,
                                                  [ref.STEPPED] * 3]
    assert [g[3] for g in got] == [1, 2, 0]
    # the open pose's sums are those of the pose before its last step: not what gsl_map_pose_info gives at the final one
    assert not np.array_equal(got[AT][6], _pose_info(means, got[AT][1], intr, depth))
    # one iteration more closes it, and nothing else about it changes
    more, _ = _check(means, _starts(3), intr, depth, max_steps=4)
    assert more[AT][3] == 2 and same_bits(more[AT][0], got[AT][0]) and same_bits(more[AT][4][:3], got[AT][4])


def test_a_plane_without_damping_is_singular():
    depth, means = tinfo.plane_case()
    query = np.full_like(depth, 2.02)
    w2cs = np.stack([np.eye(4, dtype=F32), info.w2c_of(tinfo.yaw_pose((0.0, 0.0, 0.01), 0.0))])
    got, _ = _check(means, w2cs, tinfo.PINTR, query, damping=0.0)
    for g, w in zip(got, w2cs):
        assert (g[4][:, 0] == ref.SINGULAR).all() and g[3] == 2 and g[2] == 0 and same_bits(g[1], w)
    damped, _ = _check(means, w2cs, tinfo.PINTR, query)  # with it: three directions exactly open, and they do not move
    assert not damped[0][5][:, 2:5].any() and abs(damped[0][0][2, 3] - 0.02) <= 1e-4


def test_permuted_poses_give_permuted_results_and_two_calls_the_same_bits(corner):
    intr, means, depth = corner
    w2cs = _starts(5)
    first = _run_batch(means, w2cs, intr, depth, max_trans=0.03)
    for g, w in zip(_run_batch(means, w2cs, intr, depth, max_trans=0.03), first):
        _same(g, w)
    order = [3, 0, 4, 2, 1]
    for g, p in zip(_run_batch(means, w2cs[order], intr, depth, max_trans=0.03), order):
        _same(g, first[p])
    assert len({g[4][-1, 0] for g in first}) == 3  # CONVERGED, TOO_FAR and FEW took part


def test_bad_arguments_are_refused_with_nothing_written(corner):
    intr, means, depth = corner
    lib = _lib.load_library()
    assert lib.gsl_map_align_batch_max_poses() == ALIGN_BATCH_MAX_POSES == 16
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)  # noqa: E731
    m_t, w_t, d_t = t(means), t(_starts(16).reshape(16, 16)), t(depth)
    buf = torch.full((2 * GUARD + 17 * (30 + 8 + 14 + 80),), FILL, dtype=torch.int64, device=DEV)
    at = buf.data_ptr() + 8 * GUARD
    good = dict(sums=at, work=at + 8 * 17 * 30, state=at + 8 * 17 * 38, history=at + 8 * 17 * 52)
    for k, over in [(0, {}), (17, {}), (-1, {})] + [(2, {name: None}) for name in good]:
        p = dict(good, **over)
        assert _call(lib, m_t, len(means), w_t, k, intr, d_t, 160, 120, DEFAULTS, p["sums"], p["work"], p["state"],
                     p["history"]) == BAD_ARG, (k, over)
    null = ctypes.c_void_p(None)
    assert lib.gsl_map_pose_align_batch(
        _lib.ptr(m_t), len(means), null, 2, *intr, _lib.ptr(d_t), 160, 120, float(KEEP), float(BEYOND), float(KAPPA),
        float(NEAR), 8, 1e-3, 7, 0.2, 0.3, 1e-6, 1e-5, good["sums"], good["work"], good["state"], good["history"],
        _lib.current_stream()) == BAD_ARG
    assert _call(lib, m_t, len(means), w_t, 2, intr, d_t, 160, 120, dict(DEFAULTS, max_steps=33), *good.values()) == BAD_ARG
    torch.cuda.synchronize()
    assert bool((buf == FILL).all())


def test_align_poses_of_a_map_on_the_device(corner):
    """The host layer's one buffer and its offsets: 17 poses go in two calls, and every result is align_pose's."""
    intr, means, depth = corner
    K = replica_intrinsics(160, 120)
    m = GaussianMap(160, 120, MapConfig(align=True), DEV)
    m.means[:len(means)] = torch.from_numpy(means).to(DEV)
    m.n_live = len(means)
    before = m.means.clone()
    c2ws = [torch.from_numpy(np.linalg.inv(w.astype(np.float64))) for w in _starts(17)]
    d_t = torch.from_numpy(depth)
    for steps in (8, 3):  # the second call reuses the buffer with a shorter history
        many = m.align_poses(d_t, K, c2ws, NEAR, steps=steps)
        want = bref.pose_align_batch(means, np.stack([info.w2c_of(c.numpy()) for c in c2ws]), intr, depth, KEEP, BEYOND,
                                     KAPPA, NEAR, steps, *(DEFAULTS[k] for k in ("damping", "min_used", "max_rot",
                                                                                 "max_trans", "eps_rot", "eps_trans")))
        assert len(many) == 17
        for p in (0, 1, 3, 15, 16):
            al, one, (P, work, taken, done, rows, xis, sums) = many[p], m.align_pose(d_t, K, c2ws[p], NEAR, steps=steps), want[p]
            assert same_bits(al.w2c64, one.w2c64) and same_bits(al.w2c64[:3], P) and torch.equal(al.c2w, one.c2w)
            assert (al.status, al.steps, al.used, al.tested) == (one.status, one.steps, one.used, one.tested)
            assert al.steps == taken and al.status == ref.NAMES[rows[-1, 0]] and len(al.history) == steps
            for h, o, x in zip(al.history, one.history, xis):
                assert h[:4] == o[:4] and same_bits(h[4], o[4]) and same_bits(h[4], x)
            assert al.closed == (done == 2) and (al.final is not None) == al.closed and not one.closed
            if al.closed:
                f, w = al.final, tinfo.information(sums)
                assert same_bits(f.H, w.H) and same_bits(f.g, w.g) and (f.rss, f.used, f.tested) == (w.rss, w.used, w.tested)
    assert many[0].status == "CONVERGED" and not many[0].closed and many[1].closed  # 3 steps: the map's pose stays open
    assert torch.equal(m.means, before) and m.n_live == len(means)
