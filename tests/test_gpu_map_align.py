"""GPU: gsl_map_pose_align (csrc/map_align.hip) against the numpy mirror tests/map_align_ref.py, bit for bit: the 12
float64 values of the pose, the 16 float32 values of the working copy, steps_taken, done, and every history row (four
integers and the six float64 of xi), plus the 30 sums the last iteration left.

The base case is the corner view of tests/test_map_align_cpu.py at 160x120: the map is the back-projection of one frame
(19 200 rows), the query 1 cm / 0.5 degrees away, 8 iterations, damping 1e-3.  One thing varies at a time around it:
the rows (n rows of that map spread over the image: 1 and 6 are too few, 7 is the first count that is solved,
64 / 65 and 257 / 1025 lie on either side of a wave and of one and four workgroups of k_map_pose_info), the image
(4x4 -- one 2x2 block of inner pixels, too few rows by construction --, 5x3, 33x17, each with the map of its own size),
the iterations (1, 2, 8) and the damping (0 and 1e-3).  Each of the five statuses is reached by a case made for it.
Two calls give the same bits; means, depth, the start pose and guard words around every buffer keep theirs; and
gsl_map_pose_info, called afterwards at the final float32 pose, gives the mirror's 30 integers -- the launcher both
entry points share changed nothing.  Last, GaussianMap.align_pose on the device against the mirror: the host layer's one
buffer and its offsets."""
import math

import numpy as np
import pytest
import torch

from gsplatloc_amd import _lib
from gsplatloc_amd.mapping import ALIGN_STATUS, GaussianMap, MapConfig
from gsplatloc_amd.synthetic import replica_intrinsics, room_depth
from tests import map_align_ref as ref
from tests import map_info_ref as info
from tests import test_map_info_cpu as tinfo
from tests.test_map_align_cpu import AT_MAP, DEFAULTS, KAPPA, KEEP, BEYOND, NEAR, QUERIES, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
FILL = 0x7F7F7F7F7F7F7F7F
GUARD = 8  # 8-byte words on either side of every buffer
ROWS = [1, 6, 7, 64, 65, 257, 1025, 19200]
IMAGES = [(4, 4), (5, 3), (33, 17), (160, 120)]


def _guarded(words):
    buf = torch.full((2 * GUARD + words,), FILL, dtype=torch.int64, device=DEV)
    return buf, buf[GUARD:GUARD + words]


def _run(means, w2c, intr, depth, **over):
    """The entry point on buffers inside guard words.  The inputs and the guards keep their bits.  Returns what
    tests/map_align_ref.pose_align returns."""
    a = dict(DEFAULTS, **over)
    lib, ptr, st = _lib.load_library(), _lib.ptr, _lib.current_stream()
    n, (h, w), steps = means.shape[0], depth.shape, a["max_steps"]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)  # noqa: E731
    start = np.asarray(w2c, F32).reshape(16)
    m_t, w_t, d_t = t(means), t(start), t(depth)
    bufs = [_guarded(words) for words in (info.VALUES, 8, 14, steps * 10)]
    sums, work, state, history = (b[1] for b in bufs)
    _lib.check(lib.gsl_map_pose_align(ptr(m_t), n, ptr(w_t), *(float(v) for v in intr), ptr(d_t), w, h, float(KEEP),
                                      float(BEYOND), float(KAPPA), float(NEAR), steps, a["damping"], a["min_used"],
                                      a["max_rot"], a["max_trans"], a["eps_rot"], a["eps_trans"], sums.data_ptr(),
                                      work.data_ptr(), state.data_ptr(), history.data_ptr(), st), "gsl_map_pose_align")
    torch.cuda.synchronize()
    for buf, inner in bufs:
        assert bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + inner.numel():] == FILL).all())
    for dev, host in ((m_t, means), (w_t, start), (d_t, depth)):  # the inputs are only read
        assert np.array_equal(dev.cpu().numpy().view(np.uint32), np.ascontiguousarray(host).view(np.uint32))
    state, history = state.cpu().numpy(), history.cpu().numpy().reshape(steps, 10)
    return (state[:12].view(np.float64).reshape(3, 4).copy(), work.cpu().numpy().view(F32).reshape(4, 4).copy(),
            int(state[12]), int(state[13]), history[:, :4].copy(), history[:, 4:].copy().view(np.float64),
            sums.cpu().numpy().copy())


def _same(got, want):
    names = ("pose", "working copy", "steps_taken", "done", "history integers", "history xi", "sums")
    for name, g, w in zip(names, got, want):
        if isinstance(w, np.ndarray):
            assert same_bits(g, w), (name, g, w)
        else:
            assert g == w, (name, g, w)


@pytest.fixture(scope="module")
def views():
    """Per image size: (intr, means of the map's frame, the query's depth)."""
    out = {}
    for w, h in IMAGES:
        K = replica_intrinsics(w, h)
        intr = tinfo.intrinsics(K)
        d_map = room_depth(w, h, K, torch.from_numpy(AT_MAP).float()).numpy()
        d_query = room_depth(w, h, K, torch.from_numpy(QUERIES["1cm0.5deg"]).float()).numpy()
        out[(w, h)] = (intr, tinfo.back_projection(d_map, intr, AT_MAP), d_query)
    return out


START = info.w2c_of(AT_MAP)


def _mirror(means, w2c, intr, depth, **over):
    a = dict(DEFAULTS, **over)
    return ref.pose_align(means, w2c, intr, depth, KEEP, BEYOND, KAPPA, NEAR, a["max_steps"], a["damping"],
                          a["min_used"], a["max_rot"], a["max_trans"], a["eps_rot"], a["eps_trans"])


def _rows(means, n):
    """n rows of the 160x120 map spread over the image, from pixel (5, 10) on (not the border, which no count uses)."""
    if n == len(means):
        return means
    return np.ascontiguousarray(means[1605::(len(means) - 1700) // n][:n])


@pytest.mark.parametrize("n", ROWS)
def test_the_rows(n, views):
    intr, means, depth = views[(160, 120)]
    some = _rows(means, n)
    assert some.shape == (n, 3)
    want = _mirror(some, START, intr, depth)
    if n < 7:
        assert (want[4][:, 0] == ref.FEW).all()
    elif n == 7:
        assert want[4][0, 0] == ref.STEPPED and want[4][0, 1] == 7  # all seven used: solved
    elif n >= 257:
        assert want[2] >= 1 and want[4][0, 1] > n // 2
    if n == 19200:
        assert want[4][-1, 0] == ref.CONVERGED and want[2] <= 4
    _same(_run(some, START, intr, depth), want)


@pytest.mark.parametrize("size", IMAGES[:-1])
def test_the_images(size, views):
    intr, means, depth = views[size]
    want = _mirror(means, START, intr, depth)
    if size == (4, 4):
        assert (want[4][:, 0] == ref.FEW).all() and 0 < want[4][0, 2] <= 4  # its inner pixels are one 2x2 block
    _same(_run(means, START, intr, depth), want)


@pytest.mark.parametrize("damping", [0.0, 1e-3])
@pytest.mark.parametrize("steps", [1, 2, 8])
def test_the_iterations_and_the_damping(steps, damping, views):
    intr, means, depth = views[(160, 120)]
    want = _mirror(means, START, intr, depth, max_steps=steps, damping=damping)
    assert want[4].shape == (steps, 4) and want[2] == min(steps, want[2])
    if steps == 1:
        assert want[4][0, 0] == ref.STEPPED and want[3] == 0 and want[2] == 1
    _same(_run(means, START, intr, depth, max_steps=steps, damping=damping), want)


def test_every_status_is_reached(views):
    intr, means, depth = views[(160, 120)]
    plane_depth, plane_means = tinfo.plane_case()
    plane_query = np.full_like(plane_depth, 2.02)
    cases = {
        ref.CONVERGED: (means, START, intr, depth, {}),
        ref.STEPPED: (means, START, intr, depth, dict(max_steps=2, eps_rot=0.0, eps_trans=0.0)),
        ref.FEW: (_rows(means, 6), START, intr, depth, {}),
        ref.SINGULAR: (plane_means, np.eye(4, dtype=F32), tinfo.PINTR, plane_query, dict(damping=0.0)),
        ref.TOO_FAR: (means, START, intr, depth, dict(max_trans=1e-3)),
    }
    assert sorted(cases) == list(range(len(ALIGN_STATUS)))
    for status, (m, w2c, k, d, over) in cases.items():
        want = _mirror(m, w2c, k, d, **over)
        assert want[4][-1, 0] == status, (ref.NAMES[status], want[4][:, 0])
        got = _run(m, w2c, k, d, **over)
        _same(got, want)
        if status in (ref.FEW, ref.SINGULAR, ref.TOO_FAR):  # the pose keeps its bits, every row repeats the status
            assert (got[4][:, 0] == status).all() and got[2] == 0 and got[3] == 1
            assert same_bits(got[1], np.asarray(w2c, F32).reshape(4, 4))
            assert same_bits(got[0], np.asarray(w2c, F32).reshape(4, 4)[:3].astype(np.float64))
    # a plane with the damping: three directions exactly open, and they do not move
    want = _mirror(plane_means, np.eye(4, dtype=F32), tinfo.PINTR, plane_query)
    got = _run(plane_means, np.eye(4, dtype=F32), tinfo.PINTR, plane_query)
    _same(got, want)
    assert not got[5][:, 2:5].any() and abs(got[0][2, 3] - 0.02) <= 1e-4


def test_two_calls_give_the_same_bits_and_the_sums_entry_point_is_unchanged(views):
    intr, means, depth = views[(160, 120)]
    first, second = _run(means, START, intr, depth), _run(means, START, intr, depth)
    _same(second, first)
    assert first[4][-1, 0] == ref.CONVERGED
    # gsl_map_pose_info at the final float32 pose: the mirror's 30 integers, and those the last iteration left
    lib, ptr = _lib.load_library(), _lib.ptr
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)  # noqa: E731
    m_t, w_t, d_t = t(means), t(first[1].reshape(16)), t(depth)
    out = torch.full((info.VALUES,), FILL, dtype=torch.int64, device=DEV)
    _lib.check(lib.gsl_map_pose_info(ptr(m_t), len(means), ptr(w_t), *intr, ptr(d_t), 160, 120, float(KEEP), float(BEYOND),
                                     float(KAPPA), float(NEAR), ptr(out), _lib.current_stream()), "gsl_map_pose_info")
    got = out.cpu().numpy()
    assert np.array_equal(got, info.pose_info(means, first[1], intr, depth, KEEP, BEYOND, KAPPA, NEAR))
    assert np.array_equal(got, first[6])


def test_align_pose_of_a_map_on_the_device(views):
    intr, means, depth = views[(160, 120)]
    K = replica_intrinsics(160, 120)
    m = GaussianMap(160, 120, MapConfig(align=True), DEV)
    m.means[:len(means)] = torch.from_numpy(means).to(DEV)
    m.n_live = len(means)
    before = m.means.clone()
    for steps in (8, 3):  # the second call reuses the buffer: rows of the first call beyond its own are not read
        al = m.align_pose(torch.from_numpy(depth), K, torch.from_numpy(AT_MAP), NEAR, steps=steps)
        P, work, taken, done, rows, xis, _ = _mirror(means, START, intr, depth, max_steps=steps)
        assert same_bits(al.w2c64[:3], P) and al.steps == taken and al.status == ref.NAMES[rows[-1, 0]]
        assert (al.used, al.tested) == (int(rows[-1, 1]), int(rows[-1, 2])) and len(al.history) == steps
        for h, r, x in zip(al.history, rows, xis):
            assert (h[0], h[1], h[2], h[3]) == (ref.NAMES[r[0]], r[1], r[2], float(r[3]) / 2.0 ** 20) and same_bits(h[4], x)
        assert al.c2w.is_cuda and same_bits(al.c2w.cpu().numpy(), np.linalg.inv(al.w2c64).astype(F32))
    d = al.c2w.cpu().numpy().astype(np.float64) - QUERIES["1cm0.5deg"]
    assert np.linalg.norm(d[:3, 3]) < 1e-3 and math.sqrt(float((d[:3, :3] ** 2).sum())) < 1e-3  # 3 steps: near the query
    assert torch.equal(m.means, before) and m.n_live == len(means)
