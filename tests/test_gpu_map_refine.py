"""GPU: gsl_map_refine (csrc/map_refine.hip) against the numpy mirror tests/map_refine_ref.py on given arrays, bit for
bit on means, colours, weights and counters[0]; GaussianMap.refine with the insertion and a removal on real kernels.

Row counts: 1; 63 / 64 / 65 around one wave; 255 / 256 / 257 around one workgroup; 1000 (four workgroups, the last one
partial); 4099 (17 workgroups, three rows in the last).  Images: 7x5, 33x17 and 2x2 (the smallest the entry point
takes: every row reads the same four pixels).  Poses: the exact quarter turn and the general pose of
tests/test_gpu_map_view.py.  Rows: a random cloud about a wavy surface with a step, holes (0, negative, NaN, inf) and
rows up to 12 % off it -- so that the gate passes some and refuses others -- reaching a pixel beyond every border, with
NaN / inf rows mixed in and weights on both sides of every cap; and the hand-made rows of tests/test_map_refine_cpu.py.
Variants: with and without an rgb image, max_weight 1, 2, 64.

Every call runs on arrays with GUARD_ROWS sentinel rows behind the rows it is given (and a sentinel behind the
counter): those, and depth, rgb and w2c, keep their bits.  The rule has no rounding freedom on given float32 inputs:
everything is compared for equality."""
import numpy as np
import pytest
import torch

from gsplatloc_amd import _lib
from gsplatloc_amd.mapping import GaussianMap, MapConfig
from tests import map_free_ref
from tests import map_refine_ref as ref
from tests import test_map_refine_cpu as cpu
from tests.test_abi import prototypes
from tests.test_gpu_map_view import _exact_pose, _pose, _world

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
ROWS = [1, 63, 64, 65, 255, 256, 257, 1000, 4099]
IMAGES = [(7, 5), (33, 17), (2, 2)]
POSES = {"exact": _exact_pose, "general": _pose}
SENTINEL, GUARD_ROWS = -7.25, 64
NEAR, KEEP = 0.5, ref.keep_of(0.05)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _intr(w, h):
    return tuple(float(F32(a)) for a in (0.6 * w + 1.7, 0.7 * h + 2.3, w / 2 - 0.3, h / 2 + 0.2))


def _surface(w, h, seed):
    """depth [h,w]: a wavy surface around 2 m with a step down its middle column and, in images with room for them, one
    hole of every kind; rgb [h,w,3] in 0..255."""
    rng = np.random.default_rng(seed)
    v, u = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    depth = (2.0 + 0.04 * np.sin(0.7 * u) + 0.03 * np.cos(0.9 * v) + 0.5 * (u > w // 2 + 1)).astype(F32)
    if w * h >= 35:
        for value in (0.0, -1.0, np.nan, np.inf):
            depth[rng.integers(0, h), rng.integers(0, w)] = value
    return depth, rng.uniform(0.0, 255.0, (h, w, 3)).astype(F32)


def _cloud(n, w, h, c2w, depth, seed):
    """(means [n,3] float32 in the world, weights [n] int32): rows about the surface, as the module's text says."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = _intr(w, h)
    u, v = rng.uniform(-1.0, w, n), rng.uniform(-1.0, h, n)
    near = np.nan_to_num(ref.nearest_depth(depth, u, v), nan=2.0, posinf=2.0)
    z = np.where(near > 0, near, 2.0) * rng.choice([1.0, 0.999, 1.001, 0.97, 1.03, 0.88, 1.12], n)
    p = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], -1)
    special = [[np.nan, 0.0, 2.0], [0.0, 0.0, np.nan], [np.inf, 0.0, 2.0], [0.0, -np.inf, 2.0], [0.0, 0.0, np.inf],
               [0.0, 0.0, -2.0], [0.0, 0.0, NEAR], [0.0, 0.0, 0.0]]
    where = rng.permutation(n)[:min(n // 4, len(special))]
    p[where] = np.array(special)[:len(where)]
    weights = rng.choice([1, 2, 3, 63, 64, 65, 1000], n).astype(np.int32)
    with np.errstate(invalid="ignore"):
        return _world(p, c2w), weights


def _run(means, colors, weights, w2c, cam, intr, depth, rgb, keep, near, max_weight):
    """The entry point on copies with GUARD_ROWS sentinel rows behind them; the arrays afterwards, on the host, and what
    the read-only inputs hold afterwards."""
    lib, ptr, st = _lib.load_library(), _lib.ptr, _lib.current_stream()
    n = len(means)
    h, w = depth.shape

    def padded(a, fill, dtype):
        out = torch.full((n + GUARD_ROWS,) + a.shape[1:], fill, dtype=dtype, device=DEV)
        out[:n] = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        return out

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    m_t, c_t, w_t = padded(means, SENTINEL, torch.float32), padded(colors, SENTINEL, torch.float32), padded(weights, -77, torch.int32)
    p_t, d_t, r_t = t(np.asarray(w2c, F32)), t(depth), None if rgb is None else t(rgb)
    counters = torch.full((9,), -5, dtype=torch.int32, device=DEV)
    _lib.check(lib.gsl_map_refine(ptr(m_t), None if rgb is None else ptr(c_t), ptr(w_t), n, ptr(p_t),
                                  *(float(a) for a in cam), *intr, ptr(d_t), ptr(r_t), w, h, float(keep), float(near),
                                  int(max_weight), ptr(counters), st), "gsl_map_refine")
    torch.cuda.synchronize()
    return dict(means=m_t.cpu().numpy(), colors=c_t.cpu().numpy(), weights=w_t.cpu().numpy(),
                counters=counters.cpu().numpy(), w2c=p_t.cpu().numpy(), depth=d_t.cpu().numpy(),
                rgb=None if rgb is None else r_t.cpu().numpy())


def _check(means, colors, weights, w2c, cam, intr, depth, rgb, keep, near, max_weight, what):
    want = ref.refine(means, colors, weights, w2c, cam, intr, depth, rgb, keep, near, max_weight)
    got = _run(means, colors, weights, w2c, cam, intr, depth, rgb, keep, near, max_weight)
    n = len(means)
    assert got["counters"][0] == want["count"] and (got["counters"][1:] == -5).all(), what
    assert np.array_equal(_bits(got["means"][:n]), _bits(want["means"])), what
    assert np.array_equal(got["weights"][:n], want["weights"]), what
    # the colours: the mirror's with an image, the input's bits without one
    assert np.array_equal(_bits(got["colors"][:n]), _bits(want["colors"] if rgb is not None else colors)), what
    # rows the rule leaves alone keep every bit (NaN payloads included)
    alone = ~want["refined"]
    assert np.array_equal(_bits(got["means"][:n][alone]), _bits(means[alone])), what
    assert np.array_equal(got["weights"][:n][alone], weights[alone]), what
    assert np.array_equal(_bits(got["colors"][:n][alone]), _bits(colors[alone])), what
    # the guard rows behind the arrays, and the inputs that are only read
    assert (got["means"][n:] == SENTINEL).all() and (got["colors"][n:] == SENTINEL).all(), what
    assert (got["weights"][n:] == -77).all(), what
    assert np.array_equal(_bits(got["depth"]), _bits(depth)) and np.array_equal(_bits(got["w2c"]), _bits(w2c)), what
    assert rgb is None or np.array_equal(_bits(got["rgb"]), _bits(rgb)), what
    return want


@pytest.mark.parametrize("pose", sorted(POSES))
@pytest.mark.parametrize("n", ROWS)
def test_refine_against_the_mirror(n, pose):
    c2w = POSES[pose]()
    w2c, cam = ref.w2c_of(c2w), ref.cam_of(c2w)
    shares = []
    for w, h in IMAGES:
        depth, rgb = _surface(w, h, seed=w)
        means, weights = _cloud(n, w, h, c2w, depth, seed=100 * n + w)
        colors = np.random.default_rng(n).uniform(0.0, 1.0, (n, 3)).astype(F32)
        for image in (None, rgb):
            for max_weight in (1, 2, 64):
                want = _check(means, colors, weights, w2c, cam, _intr(w, h), depth, image, KEEP, NEAR, max_weight,
                              (n, pose, w, h, image is not None, max_weight))
        shares.append(want["refined"].mean())
        if n >= 1000:  # the cloud is what it says: the gate passes some rows and refuses others
            assert 0.02 < shares[-1] < 0.9, (w, h, shares[-1])  # (2x2: a ninth of the rows are inside at all)
            assert (want["weights"][want["refined"]] == np.minimum(weights[want["refined"]].astype(np.int64) + 1, 64)).all()
    if n >= 64:
        assert max(shares) > 0


def test_more_rows_than_one_trip_of_the_grid():
    """The grid is capped (REFINE_MAX_BLOCKS workgroups of 256 rows): one row more than a trip holds, so that workgroup
    0 alone makes a second one, and a count at which the last workgroups make one trip fewer than the first."""
    import os
    import re

    src = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "map_refine.hip")).read()
    trip = 256 * int(re.search(r"REFINE_MAX_BLOCKS = (\d+);", src).group(1))
    c2w, (w, h) = _pose(), (33, 17)
    depth, rgb = _surface(w, h, seed=w)
    for n in (trip + 1, trip + 256 * 37 + 5):
        means, weights = _cloud(n, w, h, c2w, depth, seed=n)
        colors = np.random.default_rng(n).uniform(0.0, 1.0, (n, 3)).astype(F32)
        args = (ref.w2c_of(c2w), ref.cam_of(c2w), _intr(w, h), depth, rgb, KEEP, NEAR, 64)
        means[n - 1] = means[np.flatnonzero(ref.refine(means, colors, weights, *args)["refined"])[0]]  # the last row moves
        want = _check(means, colors, weights, *args, n)
        assert want["refined"][n - 1] and want["count"] > n // 4


def test_the_hand_made_rows():
    """The rows of tests/test_map_refine_cpu.py on the device: the quarter-pixel rows of a flat image (nothing moves,
    every weight goes up), one bad pixel of the four and the thresholds, the borders of the image, rows a step outside
    it, the near plane and rows that are not numbers."""
    step = lambda x, to: float(np.nextafter(F32(x), F32(to)))  # noqa: E731
    eye, origin, intr = cpu.EYE, cpu.ORIGIN, cpu.INTR

    def go(points, depth, keep=0.5, near=cpu.NEAR, weights=None, rgb=None, max_weight=64):
        p = np.array(points, F32).reshape(-1, 3)
        w = np.ones(len(p), np.int32) if weights is None else np.array(weights, np.int32)
        col = np.full((len(p), 3), 0.5, F32)
        return _check(p, col, w, eye, origin, intr, depth, rgb, F32(keep), near, max_weight, (points, depth))

    rows = cpu.hand_made_rows()
    r = go(rows, cpu.FLAT, rgb=np.full((cpu.RH, cpu.RW, 3), 255.0, F32))
    assert r["refined"].all() and np.array_equal(_bits(r["means"]), _bits(rows)) and (r["weights"] == 2).all()
    one = [cpu._p(2.5, 1.25)]
    for vv, uu in ((1, 2), (1, 3), (2, 2), (2, 3)):
        for value, refined in ((0.0, False), (-1.0, False), (np.nan, False), (np.inf, False), (-np.inf, False),
                               (step(4.0, 9), False), (step(1.0, 0), False), (4.0, True), (1.0, True)):
            d = cpu.FLAT.copy()
            d[vv, uu] = value
            assert go(one, d)["refined"].tolist() == [refined], (vv, uu, value)
    last = np.full((cpu.RH, cpu.RW), 2.5, F32)
    last[:, cpu.RW - 1] = 2.0
    last[cpu.RH - 1, :] = 2.0
    r = go([cpu._p(cpu.RW - 1, 1.5), cpu._p(2.25, cpu.RH - 1), cpu._p(cpu.RW - 1, cpu.RH - 1), cpu._p(0.0, 0.0),
            cpu._p(3.0, 2.0)], last)
    assert r["refined"].all() and r["a"].tolist() == [1.0, 0.25, 1.0, 0.0, 0.0] and r["d"][:3].tolist() == [2.0] * 3
    deep = np.full((cpu.RH, cpu.RW), 4.0, F32)
    outside = [cpu._first_outside(axis, limit, sign)[0]
               for axis, limit, sign in ((0, cpu.RW - 1, 1), (0, 0.0, -1), (1, cpu.RH - 1, 1), (1, 0.0, -1))]
    assert not go(outside, deep)["refined"].any()
    assert go([[3.0, 0.0, 4.0], [-2.0, 0.0, 4.0], [0.0, 2.0, 4.0], [0.0, -1.0, 4.0]], deep)["refined"].all()
    assert go([cpu._p(2.5, 1.5)], cpu.FLAT, near=2.0)["refined"].tolist() == [False]
    nan, inf = np.nan, np.inf
    assert not go([[nan, 0, 2], [0, nan, 2], [0, 0, nan], [inf, 0, 2], [0, -inf, 2], [0, 0, inf], [0, 0, -inf],
                   [0, 0, -2.0], [0, 0, 0.0], [nan, nan, nan]], cpu.FLAT)["refined"].any()
    r = go([cpu._p(2.5, 1.5)] * 4, np.full((cpu.RH, cpu.RW), 3.0, F32), weights=[2, 3, 4, 9], max_weight=4)
    assert r["weights"].tolist() == [3, 4, 4, 4]


def test_the_oblique_plane_on_the_device():
    depth, rows, truth = cpu.oblique_case()
    w = np.zeros(len(rows), np.int32)
    r = _check(rows, np.zeros_like(rows), w, cpu.EYE, cpu.ORIGIN, cpu.OINTR, depth, None, cpu.OKEEP, cpu.NEAR, 64,
               "oblique")
    assert r["refined"].all()


def test_bad_arguments_are_refused_without_a_launch(repo_root):
    """The refusals of tests/test_map_refine_cpu.py with device pointers, one per check: nothing is written."""
    lib = _lib.load_library()
    params = prototypes(repo_root)[cpu.REFINE][1]
    buf = torch.full((4096,), 0x5A, dtype=torch.uint8, device=DEV)
    for what, over in cpu.REFUSED:
        named = dict(cpu.GOOD, **over)
        assert lib.gsl_map_refine(*cpu.refine_args(params, named, buf.data_ptr())) == cpu.BAD_ARG, what
    torch.cuda.synchronize()
    assert bool((buf == 0x5A).all())


def test_gaussian_map_inserts_refines_and_removes():
    """insert_frame, refine and remove_seen_through on real kernels: the refined rows and the weights are the
    mirror's, and the weights follow their rows through the removal."""
    frames = cpu.noisy_sequence(3)
    w, h = cpu.NW, cpu.NH
    K = cpu.replica_intrinsics(w, h)
    intr = tuple(float(F32(a)) for a in (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))
    m = GaussianMap(w, h, MapConfig(refine=True, free_rho=0.05, capacity=w * h + 100), DEV)
    rgb = torch.randint(0, 255, (h, w, 3), generator=torch.Generator().manual_seed(2)).float()
    assert m.refine(frames[0][0], None, K, frames[0][1], 0.01) == 0  # an empty map
    assert m.insert_frame(frames[0][0], rgb, K, frames[0][1]) == (w * h, w * h)
    n = m.n_live
    assert (m.weights[:n] == 1).all()
    means, colors, weights = m.points.cpu().numpy(), m.point_colors.cpu().numpy(), m.weights[:n].cpu().numpy()
    for (depth, pose), image in ((frames[1], None), (frames[2], rgb)):
        want = ref.refine(means, colors, weights, ref.w2c_of(pose.numpy()), ref.cam_of(pose.numpy()), intr,
                          depth.numpy(), None if image is None else image.numpy(), ref.keep_of(0.05), 0.01, 64)
        assert m.refine(depth, image, K, pose, 0.01) == want["count"] > n // 2
        assert np.array_equal(_bits(m.points.cpu().numpy()), _bits(want["means"]))
        assert np.array_equal(m.weights[:n].cpu().numpy(), want["weights"])
        assert np.array_equal(_bits(m.point_colors.cpu().numpy()), _bits(want["colors"]))
        means, weights, colors = want["means"], want["weights"], want["colors"]
    assert sorted(set(weights.tolist())) == [1, 2, 3]
    # a block of rows pulled to 60 % of their distance: the frame sees through them, they go, the weights follow
    m.means[1000:1200] *= 0.6
    means = m.points.cpu().numpy()
    pose = frames[0][1]
    kept = map_free_ref.select(means, ref.w2c_of(pose.numpy()), intr, frames[0][0].numpy(), F32(m._free_keep), 1, 0.01)
    removed, stay = m.remove_seen_through(frames[0][0], K, pose, 0.01)
    assert removed == n - len(kept["ids"]) > 0 and stay == len(kept["ids"])
    assert np.array_equal(m.survivors.cpu().numpy(), kept["ids"])
    assert np.array_equal(m.weights[:stay].cpu().numpy(), weights[kept["ids"]])
    assert np.array_equal(_bits(m.points.cpu().numpy()), _bits(means[kept["ids"]]))
