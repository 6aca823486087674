"""GPU: gsl_map_score (csrc/map_score.hip) against the numpy mirror tests/map_score_ref.py on given arrays, bit for bit,
and GaussianMap.score_poses.

Pose, intrinsics and depth image are those of tests/test_gpu_map_free.py -- a quarter turn and a dyadic translation,
power-of-two intrinsics, dyadic depths, keep = 0.9375 and here beyond = 1.0625 -- so that the hand-made rows sit on their
thresholds on the device as well.  The two images are windows of that depth image, the principal point moved by the
window's whole-pixel origin (still exact): 7x5 at (10, 7) and 33x17 at (0, 0).  Both hold pixels of the patch at exactly
2 m and of the patch one float32 step above; stamped into them are a pixel one step BELOW 2 m and pixels with depth 0,
NaN, +inf and -1.

The hand-made rows (at pose 0; their verdicts are asserted on the mirror): z == d * keep and z == d * beyond agree, the
same z against the pixel a step above is in front, against the pixel a step below behind; u = -0.5 and v = -0.5 round
to -0 and are column / line 0, 2^-17 px further out they are outside; u = width - 0.5 and v = height - 0.5 round to the
even width - 1 / height - 1 (both sizes are odd) and are inside, 2^-17 px further they are outside; z == near is
untested; NaN / inf rows, a row behind the camera and rows on the pixels without depth are untested.  The rest is a
random cloud that straddles the frustum.

Row counts: 1; 63 / 64 / 65 around one wave; 255 / 256 / 257 around one workgroup; one full sweep of the capped grid
plus 1 and two sweeps plus 3 (the grid-stride loop runs 2 and 3 trips; cap and workgroup size are read from the
source).  Pose counts 1, 2, 63 and 64: the base pose and translations by multiples of 2^-4.  counts is handed over filled
with 0x7f bytes, with a guard region behind it.  Every refusal of tests/test_map_score_cpu.py is repeated with device
pointers: nothing is written."""
import os
import re

import numpy as np
import pytest
import torch

from gsplatloc_amd import _lib
from gsplatloc_amd.mapping import GaussianMap, MapConfig
from gsplatloc_amd.synthetic import replica_intrinsics, room_depth
from tests import map_score_ref as ref
from tests.test_gpu_map_free import D_STEP, EINTR, EKEEP, NEAR, _exact_depth, _exact_pose, _world
from tests.test_gpu_map_view import _pose
from tests.test_map_score_cpu import BAD_ARG, FN, GOOD, REFUSED, call_with

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
EBEYOND = F32(1.0625)
D_BELOW = float(np.nextafter(F32(2.0), F32(0)))  # 2 - 2^-23: times 1.0625 it rounds to 2.125 - 2^-22
FILL = 0x7F7F7F7F
IMAGES = {"7x5": (7, 5, 10, 7), "33x17": (33, 17, 0, 0)}  # width, height, the window's origin in the 64x48 image
SMALL_ROWS = [1, 63, 64, 65, 255, 256, 257]
POSES = [1, 2, 63, 64]


def _grid():
    """(cap of the grid in workgroups, threads per workgroup) as csrc/map_score.hip names them."""
    src = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "map_score.hip")).read()
    cap = int(re.search(r"constexpr int SCORE_MAX_BLOCKS = (\d+);", src).group(1))
    threads = int(re.search(r"constexpr int SCORE_THREADS = (\d+);", src).group(1))
    return cap, threads


CAP, THREADS = _grid()
SWEEP = CAP * THREADS
assert THREADS == 256 and SMALL_ROWS[-3:] == [THREADS - 1, THREADS, THREADS + 1]
CASES = [(n, k, image) for image in IMAGES for k in POSES for n in SMALL_ROWS] + \
        [(SWEEP + 1, 1, "33x17"), (SWEEP + 1, 64, "33x17"), (2 * SWEEP + 3, 1, "33x17"), (2 * SWEEP + 3, 64, "33x17"),
         (SWEEP + 1, 2, "7x5"), (2 * SWEEP + 3, 63, "7x5")]


def _image(name):
    """(depth [h,w] float32, intrinsics, pixels by role).  Local pixel (c, r) is pixel (u0 + c, v0 + r) of the 64x48
    image: the patch at 2 m is its columns 4 .. 10, the patch a step above its columns 16 .. 22, lines 4 .. 10 both."""
    w, h, u0, v0 = IMAGES[name]
    d = _exact_depth()[v0:v0 + h, u0:u0 + w].copy()
    px = dict(flat=(10 - u0, 8 - v0), above=(16 - u0, 8 - v0), below=(w - 2, h - 1), zero=(1, h - 1), nan=(2, h - 1),
              inf=(3, h - 1), neg=(4, h - 1))
    for role, value in (("below", D_BELOW), ("zero", 0.0), ("nan", np.nan), ("inf", np.inf), ("neg", -1.0)):
        d[px[role][1], px[role][0]] = value
    assert d[px["flat"][1], px["flat"][0]] == 2.0 and d[px["above"][1], px["above"][0]] == F32(D_STEP)
    return d, (EINTR[0], EINTR[1], EINTR[2] - u0, EINTR[3] - v0), px


def _specials(name):
    """Hand-made rows in the camera frame of pose 0 and the verdict the rule gives each."""
    d, intr, px = _image(name)
    h, w = d.shape
    at = lambda u, v, z: [(u - intr[2]) / 64.0 * z, (v - intr[3]) / 64.0 * z, z]  # noqa: E731
    eps = 2.0 ** -17
    mid_c, mid_r = 2, 1  # a pixel of the sloping part (2 m and more): a row at 1 m is in front of it
    rows = [(at(*px["flat"], 1.875), "agree"),  # z == d * keep
            (at(*px["above"], 1.875), "front"),  # d * keep is one step above z
            (at(*px["flat"], 2.125), "agree"),  # z == d * beyond
            (at(*px["below"], 2.125), "behind"),  # d * beyond is one step below z
            (at(*px["below"], 1.875), "agree"), (at(*px["above"], 2.125), "agree"),
            (at(-0.5, mid_r, 1.0), "front"), (at(-0.5 - eps, mid_r, 1.0), "untested"),
            (at(mid_c, -0.5, 1.0), "front"), (at(mid_c, -0.5 - eps, 1.0), "untested"),
            (at(w - 0.5, mid_r, 1.0), "front"), (at(w - 0.5 + eps, mid_r, 1.0), "untested"),
            (at(0, h - 0.5, 1.0), "front"), (at(0, h - 0.5 + eps, 1.0), "untested"),
            # (the world z is the camera's + 2: a step of 2^-20 survives that sum, one float32 step of 0.5 would not)
            (at(mid_c, mid_r, NEAR), "untested"), (at(mid_c, mid_r, NEAR + 2.0 ** -20), "front"),
            (at(*px["zero"], 1.0), "untested"), (at(*px["nan"], 1.0), "untested"), (at(*px["inf"], 1.0), "untested"),
            (at(*px["neg"], 1.0), "untested"),
            ([0.0, 0.0, -1.0], "untested"), ([np.nan, 0.0, 1.0], "untested"), ([0.0, 0.0, np.nan], "untested"),
            ([np.inf, 0.0, 1.0], "untested"), ([0.0, -np.inf, 1.0], "untested"), ([0.0, 0.0, np.inf], "untested"),
            ([0.0, 0.0, -np.inf], "untested")]
    return np.array([r for r, _ in rows]), [v for _, v in rows]


def _poses(k):
    """k camera-to-world poses: the exact pose, then translations of it by multiples of 2^-4 (the inverse is exact)."""
    out = []
    for i in range(k):
        c2w = _exact_pose().copy()
        c2w[:3, 3] += np.array([(i % 4), -((i // 4) % 4), ((i // 16) % 4) - 1.0 * (i > 0)]) / 16.0
        out.append(c2w)
    return np.stack(out)


def _cloud(n, name):
    """(means [n,3] float32 in the world, where the hand-made rows are): a cloud that straddles the frustum of pose 0."""
    d, intr, _ = _image(name)
    h, w = d.shape
    rng = np.random.default_rng(1000 * n + w)
    z = rng.uniform(0.3, 4.5, n)
    u, v = rng.uniform(-3.0, w + 2.0, n), rng.uniform(-3.0, h + 2.0, n)
    p = np.stack([(u - intr[2]) / 64.0 * z, (v - intr[3]) / 64.0 * z, z], axis=-1)
    rows, _ = _specials(name)
    where = rng.permutation(n)[:min(n, len(rows))]
    p[where] = rows[:len(where)]
    with np.errstate(invalid="ignore"):
        return _world(p, _exact_pose()), where


def _run(means, w2cs, intr, depth, keep, beyond, near):
    """The entry point on counts filled with 0x7f bytes, with a guard region behind; int64 [k,3]."""
    lib, ptr, st = _lib.load_library(), _lib.ptr, _lib.current_stream()
    n, k, (h, w) = means.shape[0], w2cs.shape[0], depth.shape
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    m_t, w_t, d_t = t(means), t(w2cs.reshape(k, 16)), t(depth)
    counts = torch.full((3 * k + 64,), FILL, dtype=torch.int32, device=DEV)
    _lib.check(lib.gsl_map_score(ptr(m_t), n, ptr(w_t), k, *(float(a) for a in intr), ptr(d_t), w, h, float(keep),
                                 float(beyond), float(near), ptr(counts), st), FN)
    torch.cuda.synchronize()
    assert bool((counts[3 * k:] == FILL).all())  # nothing behind the k rows
    for dev, host in ((m_t, means), (w_t, w2cs.reshape(k, 16)), (d_t, depth)):  # the inputs are only read
        assert np.array_equal(dev.cpu().numpy().view(np.uint32), np.ascontiguousarray(host).view(np.uint32))
    return counts[:3 * k].reshape(k, 3).cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("name", list(IMAGES))
def test_the_hand_made_rows_are_what_they_say(name):
    depth, intr, _ = _image(name)
    rows, want = _specials(name)
    with np.errstate(invalid="ignore"):
        means = _world(rows, _exact_pose())
    w2c = ref.w2c_of(_exact_pose())
    tested, agree, front, behind = ref.verdicts(means, w2c, intr, depth, EKEEP, EBEYOND, NEAR)
    got = ["untested" if not t else "front" if f else "agree" if a else "behind"
           for t, a, f, b in zip(tested, agree, front, behind)]
    assert got == want
    assert float(F32(D_BELOW) * EBEYOND) == 2.125 - 2.0 ** -22 and float(F32(D_STEP) * EKEEP) == 1.875 + 2.0 ** -22
    assert float(F32(2.0) * EBEYOND) == 2.125 and float(F32(D_BELOW) * EKEEP) == 1.875 - 2.0 ** -23
    # ... and on the device: one row per call is a count of 0 or 1 in each column
    for i in range(len(rows)):
        counts = _run(means[i:i + 1], w2c[None], intr, depth, EKEEP, EBEYOND, NEAR)
        assert counts.tolist() == [[int(tested[i]), int(agree[i]), int(front[i])]], (i, want[i])


@pytest.mark.parametrize("n,k,name", CASES)
def test_counts_against_the_mirror(n, k, name):
    depth, intr, _ = _image(name)
    means, _ = _cloud(n, name)
    w2cs = np.stack([ref.w2c_of(p) for p in _poses(k)])
    want = ref.score(means, w2cs, intr, depth, EKEEP, EBEYOND, NEAR)
    if n >= 255:  # the case is not trivial: rows of every kind at pose 0
        tested, agree, front = want[0]
        assert 0 < front < tested < n and 0 < agree < tested and tested - agree - front > 0, want[0]
    got = _run(means, w2cs, intr, depth, EKEEP, EBEYOND, NEAR)
    assert np.array_equal(got, want), (got[:4], want[:4])


def test_the_largest_legal_factors_are_taken():
    """keep == 1 and beyond == 1 (depth_rho = 0): only z == d agrees."""
    depth, intr, _ = _image("33x17")
    means, _ = _cloud(1000, "33x17")
    w2cs = np.stack([ref.w2c_of(p) for p in _poses(3)])
    want = ref.score(means, w2cs, intr, depth, F32(1.0), F32(1.0), NEAR)
    assert np.array_equal(_run(means, w2cs, intr, depth, 1.0, 1.0, NEAR), want)


def test_entry_point_rejects_bad_arguments_without_a_launch(repo_root):
    from tests.test_abi import prototypes

    lib = _lib.load_library()
    params = prototypes(repo_root)[FN][1]
    buffers = {n: torch.full((65536,), FILL, dtype=torch.int32, device=DEV) for t, n in params if "*" in t and n != "stream"}
    pointers = {n: b.data_ptr() for n, b in buffers.items()}
    for what, over in REFUSED:
        assert call_with(lib, params, dict(GOOD, **over), pointers) == BAD_ARG, what
    torch.cuda.synchronize()
    for name, b in buffers.items():
        assert bool((b == FILL).all()), name


def test_score_poses_of_a_map_filled_by_insert_frame():
    w, h = 64, 48
    K = replica_intrinsics(w, h)
    pose = torch.from_numpy(_pose(deg=17.0, t=(0.6, -0.4, 0.9))).float()
    depth = room_depth(w, h, K, pose)
    rgb = torch.randint(0, 255, (h, w, 3), generator=torch.Generator().manual_seed(3)).float()
    m = GaussianMap(w, h, MapConfig(), DEV)
    near = 0.01
    assert m.score_poses(depth, K, [pose], near).tolist() == [[0, 0, 0]] and m._score is None  # empty: no launch
    assert m.insert_frame(depth, rgb, K, pose) == (w * h, w * h)
    moved = []
    for axis, metres in ((0, 0.0), (2, -0.4), (2, 0.4), (0, 0.3), (1, -0.2)):
        step = torch.eye(4)
        step[axis, 3] = metres
        moved.append(pose @ step)
    got = m.score_poses(depth, K, torch.stack(moved), near)
    intr = tuple(float(F32(a)) for a in (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))
    w2cs = np.stack([ref.w2c_of(p.numpy()) for p in moved])
    want = ref.score(m.points.cpu().numpy(), w2cs, intr, depth.numpy(), F32(m.keep), F32(m.beyond), near)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    tested, agree, front = got[0].tolist()  # the frame's own pose: every inserted row sits at its own pixel's depth
    assert front == 0 and agree == tested > 0
    assert got[2, 2] > 0 and got[2, 1] < got[2, 0]  # from 0.4 m further on, the wall ahead is nearer than observed
    assert m._score["counts"].shape == (64, 3) and m._score["poses"].shape == (64, 16)
    assert np.array_equal(m.score_poses(depth, K, moved, near), got)  # the buffers are reused, the counts zeroed again
