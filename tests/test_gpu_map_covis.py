"""GPU: gsl_map_covis (csrc/map_covis.hip) against the numpy mirror tests/map_covis_ref.py -- the counts and the rows
outside, integer for integer -- and GaussianMap.covisibility on real kernels.

The rows: 1, 63, 64, 65 (on either side of a wave), 257 (a workgroup and a row), 4097 (17 workgroups) and 131 372 (more
rows than one trip of the grid of 1024 workgroups: a wave carries its run into a second trip), against tables of 1, 3
and 300 frames -- one frame for everything is the contended word.  A 48 x 33 depth image with 15 % of its pixels
invalid (0, NaN, inf, negative); rows spread a little wider than the image, some behind the camera, some NaN, inf and
-0.0.  Origins non-decreasing as a map makes them, with rows in front of the table (-1) and behind it (n_frames) --
and shuffled, a wave that spans four origins, a wave with 64 distinct ones.  Guard words around the counts keep their
bits; the means, the origins and the depth image are not written.

The room loop (tests/map_correct_ref.room_loop, the fixture shape of tests/test_gpu_map_correct.py): eight 160 x 120
frames inserted whole at their drifted poses by the map's own kernels; ``covisibility`` of frame 7 with frames 0 .. 6 is
the integers tests/map_covis_ref.py pins."""
import numpy as np
import pytest
import torch

from gsplatloc_amd import _lib
from gsplatloc_amd.mapping import GaussianMap, MapConfig
from gsplatloc_amd.synthetic import replica_intrinsics, room_depth
from tests import map_correct_ref
from tests import map_covis_ref as ref
from tests import test_map_covis_cpu as cpu
from tests.map_score_ref import beyond_of, keep_of
from tests.test_abi import prototypes
from tests.test_map_refine_cpu import refine_args

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
ROWS = [1, 63, 64, 65, 257, 4097, 1024 * 128 + 300]
FRAMES = [1, 3, 300]
CW, CH = 48, 33
CINTR = (60.0, 55.0, 23.5, 16.0)
KEEP, BEYOND, CNEAR = float(keep_of(0.1)), float(beyond_of(0.1)), 0.25
GUARD = 8  # int32 words on either side of the counts
FILL = 0x5A5A5A5A


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _depth(rng):
    depth = rng.uniform(1.5, 2.5, (CH, CW)).astype(F32)
    bad = rng.random((CH, CW))
    depth[bad < 0.15] = 0.0
    depth[bad < 0.09] = np.nan
    depth[bad < 0.06] = np.inf
    depth[bad < 0.03] = -1.0
    return depth


def _case(n, n_frames, seed, outside=True):
    rng = np.random.default_rng(seed)
    depth = _depth(rng)
    pose = map_correct_ref.twist(3.0, 0.05, rng.normal(size=3), rng.normal(size=3))
    w2c = np.linalg.inv(pose).astype(F32)
    z = rng.uniform(1.2, 2.8, (n, 1))  # within 10 % of the surface or not: all three verdicts
    cam = np.concatenate([rng.uniform(-0.5, 0.5, (n, 1)) * z, rng.uniform(-0.4, 0.4, (n, 1)) * z, z, np.ones((n, 1))], 1)
    means = (cam @ pose.T)[:, :3].astype(F32)
    origins = np.sort(rng.integers(0, n_frames, n)).astype(np.int32)
    if n >= 63:
        k = max(n // 50, 2)
        if outside:
            origins[:k] = -1  # in front of the table and behind it: still non-decreasing
            origins[-k:] = n_frames
        for j, value in enumerate((np.nan, np.inf, -np.inf, -0.0)):
            means[(k + 5 + 7 * np.arange(8) * (j + 1)) % n, j % 3] = value
        means[n // 2, :] = -0.0
        means[n // 3] = (cam[n // 3] * [1, 1, -1, 1] @ pose.T)[:3]  # behind the camera
    return means, origins, w2c, depth


def _run(means, origins, w2c, depth, n_frames, intr=CINTR, keep=KEEP, beyond=BEYOND, near=CNEAR):
    """The entry point with the counts inside guard words.  Returns (counts int64 [n_frames,3], outside); the guards
    and the inputs keep their bits."""
    lib, ptr, st = _lib.load_library(), _lib.ptr, _lib.current_stream()
    n = len(means)
    H_, W_ = depth.shape
    buf = torch.full((2 * GUARD + 3 * n_frames,), FILL, dtype=torch.int32, device=DEV)
    counts = buf[GUARD:GUARD + 3 * n_frames]
    out = torch.full((1,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
    m_t, o_t = torch.from_numpy(means).to(DEV), torch.from_numpy(origins).to(DEV)
    w_t, d_t = torch.from_numpy(w2c.reshape(16)).to(DEV), torch.from_numpy(depth).to(DEV)
    _lib.check(lib.gsl_map_covis(ptr(m_t), ptr(o_t), n, ptr(w_t), *intr, ptr(d_t), W_, H_, keep, beyond, near, n_frames,
                                 counts.data_ptr(), ptr(out), st), "gsl_map_covis")
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + 3 * n_frames:] == FILL).all())
    assert np.array_equal(_bits(m_t.cpu().numpy()), _bits(means)) and np.array_equal(o_t.cpu().numpy(), origins)
    assert np.array_equal(_bits(d_t.cpu().numpy()), _bits(depth)) and np.array_equal(_bits(w_t.cpu().numpy()), _bits(w2c.reshape(16)))
    return counts.cpu().numpy().astype(np.int64).reshape(n_frames, 3), int(out.item())


def _check(means, origins, w2c, depth, n_frames, what):
    want, want_out = ref.covis(means, origins, w2c, CINTR, depth, F32(KEEP), F32(BEYOND), CNEAR, n_frames)
    got, got_out = _run(means, origins, w2c, depth, n_frames)
    assert got_out == want_out, (what, got_out, want_out)
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:5].tolist())
    return want, want_out


def _score(means, w2c, depth):
    lib, ptr, st = _lib.load_library(), _lib.ptr, _lib.current_stream()
    m_t, w_t, d_t = (torch.from_numpy(a).to(DEV) for a in (means, w2c.reshape(1, 16), depth))
    counts = torch.full((3,), FILL, dtype=torch.int32, device=DEV)
    _lib.check(lib.gsl_map_score(ptr(m_t), len(means), ptr(w_t), 1, *CINTR, ptr(d_t), CW, CH, KEEP, BEYOND, CNEAR,
                                 ptr(counts), st), "gsl_map_score")
    return counts.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("n_frames", FRAMES)
@pytest.mark.parametrize("n", ROWS)
def test_covis_against_the_mirror(n, n_frames):
    means, origins, w2c, depth = _case(n, n_frames, seed=n + n_frames)
    assert (np.diff(origins) >= 0).all()
    want, outside = _check(means, origins, w2c, depth, n_frames, (n, n_frames))
    if n >= 257:  # every clause is in the case
        assert outside == 2 * max(n // 50, 2)
        total = want.sum(axis=0)
        assert 0 < total[2] and 0 < total[1] and total[1] + total[2] < total[0] < n
    # the sum over the frames is what gsl_map_score leaves for the same pose, when no row is outside
    means, origins, w2c, depth = _case(n, n_frames, seed=n + n_frames, outside=False)
    want, outside = _check(means, origins, w2c, depth, n_frames, (n, n_frames, "inside"))
    assert outside == 0 and np.array_equal(want.sum(axis=0), _score(means, w2c, depth))


def test_waves_of_many_origins():
    rng = np.random.default_rng(11)
    for n, n_frames, per in ((64, 4, 16), (256, 4, 16), (100, 4, 7), (64, 64, 1), (640, 64, 1), (4097, 300, 1)):
        means, _, w2c, depth = _case(n, n_frames, seed=n + per)
        if per == 1:
            origins = (np.arange(n) % n_frames).astype(np.int32)  # every lane of a wave another origin
        elif n == 256:
            origins = (np.arange(n) // per % 4).astype(np.int32)
        else:
            origins = np.minimum(np.arange(n) // per, 3).astype(np.int32)
        want, outside = _check(means, origins, w2c, depth, n_frames, (n, n_frames, per))
        assert outside == 0 and want[:, 0].sum() > 0 and (per > 1 or (want[:, 0] > 0).sum() > min(n, n_frames) // 8)
    # shuffled origins, and origins far outside the table
    for n, n_frames in ((257, 3), (4097, 300), (1024 * 128 + 300, 48)):
        means, origins, w2c, depth = _case(n, n_frames, seed=n)
        origins = rng.permutation(origins)
        origins[rng.integers(0, n, 5)] = [2 ** 31 - 1, -2 ** 31, n_frames, -1, 2 ** 30]
        _check(means, origins, w2c, depth, n_frames, (n, n_frames, "shuffled"))


def test_one_origin_for_everything():
    """The contended word: every run of every wave adds to the same three counts."""
    n = 1024 * 128 + 300
    means, _, w2c, depth = _case(n, 5, seed=3, outside=False)
    origins = np.full(n, 2, np.int32)
    want, outside = _check(means, origins, w2c, depth, 5, "one origin")
    assert outside == 0 and not want[[0, 1, 3, 4]].any() and np.array_equal(want[2], _score(means, w2c, depth))


def test_no_rows_is_no_launch():
    lib = _lib.load_library()
    buf = torch.full((64,), 1.0e30, device=DEV)
    counts = torch.full((9,), 77, dtype=torch.int32, device=DEV)
    outside = torch.full((1,), 77, dtype=torch.int64, device=DEV)
    origins = torch.zeros(4, dtype=torch.int32, device=DEV)
    assert lib.gsl_map_covis(buf.data_ptr(), origins.data_ptr(), 0, buf.data_ptr(), *CINTR, buf.data_ptr(), 8, 8, KEEP,
                             BEYOND, CNEAR, 3, counts.data_ptr(), outside.data_ptr(), _lib.current_stream()) == 0
    torch.cuda.synchronize()
    assert counts.tolist() == [77] * 9 and outside.tolist() == [77]  # not even the zeroing launches


def test_bad_arguments_are_refused_without_a_launch(repo_root):
    """The refusals of tests/test_map_covis_cpu.py with device pointers: nothing is written."""
    lib = _lib.load_library()
    params = prototypes(repo_root)["gsl_map_covis"][1]
    buf = torch.full((4096,), 0x5A, dtype=torch.uint8, device=DEV)
    for what, over in cpu.REFUSED:
        assert lib.gsl_map_covis(*refine_args(params, dict(cpu.GOOD, **over), buf.data_ptr())) == cpu.BAD_ARG, what
    torch.cuda.synchronize()
    assert bool((buf == 0x5A).all())


# ---- GaussianMap.covisibility on the room loop --------------------------------------------------------------------------
W, H = 160, 120
K = replica_intrinsics(W, H)
NEAR = 0.01


@pytest.fixture(scope="module")
def loop():
    """(map with the eight frames inserted whole at their drifted poses, true poses, drifted poses, depth images)."""
    true, est = map_correct_ref.room_loop()
    m = GaussianMap(W, H, MapConfig(origins=True, capacity=8 * W * H), DEV)
    rgb = torch.full((H, W, 3), 100.0)
    depths = [room_depth(W, H, K, torch.from_numpy(p).float()) for p in true]
    for k in range(8):
        assert m.insert_frame(depths[k], rgb, K, torch.from_numpy(est[k]).float())[1] == W * H
    assert np.array_equal(m.origins[:m.n_live].cpu().numpy(), np.repeat(np.arange(8), W * H))
    return m, true, est, depths


@pytest.mark.parametrize("pose", ["drifted", "true"])
def test_covisibility_of_the_room_loop(loop, pose):
    m, true, est, depths = loop
    at = torch.from_numpy(est[7] if pose == "drifted" else true[7]).float()
    rows, before = m.rows_up_to(6), m.points.clone()
    assert rows == 7 * W * H
    c = m.covisibility(depths[7], K, at, NEAR, n_frames=7, rows=rows)
    print(f"[covis] room loop on the device, frame 7 at its {pose} pose: tested {c[:, 0].tolist()} agree "
          f"{c[:, 1].tolist()} front {c[:, 2].tolist()}")
    assert c.dtype == np.int64 and c.shape == (7, 3) and m.last_covis_outside == 0
    # the mirror on the map's own rows, then the pinned integers
    means, origins = m.points[:rows].cpu().numpy(), m.origins[:rows].cpu().numpy()
    intr = tuple(float(F32(a)) for a in (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))
    want, _ = ref.covis(means, origins, np.linalg.inv(at.double().numpy()).astype(F32), intr, depths[7].numpy(),
                        F32(m.keep), F32(m.beyond), NEAR, 7)
    assert np.array_equal(c, want)
    assert c[:, 0].tolist() == ref.ROOM_TESTED[pose] and c[:, 2].tolist() == ref.ROOM_FRONT[pose]
    assert c[:, 1].tolist() == ref.ROOM_AGREE[pose]
    # summed over the frames it is score_poses on the same prefix; the whole map has frame 7's own rows as well
    assert c.sum(axis=0).tolist() == m.score_poses(depths[7], K, [at], NEAR, rows=rows)[0].tolist()
    full = m.covisibility(depths[7], K, at, NEAR)
    assert full.shape == (8, 3) and np.array_equal(full[:7], c)
    assert full.sum(axis=0).tolist() == m.score_poses(depths[7], K, [at], NEAR)[0].tolist()
    # a table of seven frames over the whole map: frame 7's rows are outside it
    assert np.array_equal(m.covisibility(depths[7], K, at, NEAR, n_frames=7), c) and m.last_covis_outside == W * H
    assert torch.equal(m.points, before)  # nothing in the map is written
