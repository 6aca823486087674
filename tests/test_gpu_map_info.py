"""GPU: gsl_map_pose_info (csrc/map_info.hip) against the numpy mirror tests/map_info_ref.py on given arrays, all 30
integers, and GaussianMap.pose_information.

The grid: row counts 1; 63 / 64 / 65 around one wave; 255 / 256 / 257 around one workgroup; 1025; one trip of the capped
grid plus 1 (the grid-stride loop runs twice; cap and workgroup size are read from the source) -- times the images 2x2
(no inner pixel: every sum is 0), 3x3 (one), 7x5 and 33x17 -- times two poses, the identity and a camera turned by 3
degrees and moved by 2 cm.  An image is two planes (inverse depth linear in the pixel, what the planarity test passes up
to float32) that meet in a crease at its middle column (3x3: one plane), the 33x17 one with pixels of depth 0, NaN, +inf and -1 stamped
in.  The cloud is made of rows on, just off, in front of and behind the surface their pixel shows, at positions all over
the image and a pixel outside it, with NaN / inf rows and rows behind the camera mixed in.

The hand-made rows (identity pose: a row's camera point is the row, exactly; intrinsics 32, 32 and the image centre;
keep = 0.9375, beyond = 1.0625; their verdicts are asserted on the mirror, then one row per call on the device): on the
48x17 image of depth 2 m the inner pixels are tiled by 3x3 blocks, and a block's centre and neighbours are set so that
the row on its centre sits on a threshold -- z == d0 * keep, z == d0 * beyond and one float32 step outside either; each
neighbour in turn at d0 * keep and d0 * beyond and one step outside; each neighbour in turn NaN / +inf / 0 / -1; the
centre itself without depth; z == 64 and one step below on a block at 64 m; z == near and one step above; a crease
(a neighbour 10 cm off) under kappa = 2^-10 and kappa = 1; pixels of the border columns and lines and their inner
neighbours; halves that round to the even pixel; a row behind the camera, NaN and inf rows.  Planarity at equality has
its own image (keep = 0.5, beyond = 2): d0 = 2, neighbours 1 and 4 give |(1 + 1/4) - 1| = 1/4 = kappa / d0 at
kappa = 0.5 exactly -- used -- and one step of kappa below -- not.

out is handed over inside a buffer of guard words filled with a pattern; means, depth and w2c are compared bit for bit
after the call; two calls give the same 30 integers.  Every refusal of tests/test_map_info_cpu.py is repeated with device
pointers: nothing is written."""
import os
import re

import numpy as np
import pytest
import torch

from gsplatloc_amd import _lib
from gsplatloc_amd.mapping import GaussianMap, MapConfig, apply_twist
from gsplatloc_amd.synthetic import replica_intrinsics, room_depth
from tests import map_info_ref as ref
from tests.test_map_info_cpu import BAD_ARG, FN, GOOD, NEAR, REFUSED, call_with, intrinsics, yaw_pose

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
EKEEP, EBEYOND = F32(0.9375), F32(1.0625)
KEEP, BEYOND, KAPPA = ref.keep_of(0.05), ref.beyond_of(0.05), F32(1e-3)
FILL = 0x7F7F7F7F7F7F7F7F
GUARD = 8  # int64 words on either side of out
IMAGES = {"2x2": (2, 2), "3x3": (3, 3), "7x5": (7, 5), "33x17": (33, 17)}
up, down = (lambda x: float(np.nextafter(F32(x), F32(np.inf)))), (lambda x: float(np.nextafter(F32(x), F32(-np.inf))))


def _grid():
    """(cap of the grid in workgroups, threads per workgroup) as csrc/map_info.hip names them."""
    src = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "map_info.hip")).read()
    cap = int(re.search(r"constexpr int INFO_MAX_BLOCKS = (\d+);", src).group(1))
    threads = int(re.search(r"constexpr int INFO_THREADS = (\d+);", src).group(1))
    return cap, threads


CAP, THREADS = _grid()
assert THREADS == 256
ROWS = [1, 63, 64, 65, 255, 256, 257, 1025, CAP * THREADS + 1]
POSES = {"identity": np.eye(4), "moved": yaw_pose((0.02, -0.01, 0.005), 3.0)}


def _intr(w, h):
    return (32.0, 32.0, (w - 1) / 2.0, (h - 1) / 2.0)


def _run(means, w2c, intr, depth, keep, beyond, kappa, near):
    """The entry point on out inside guard words; int64 [30].  The inputs and the guards keep their bits."""
    lib, ptr, st = _lib.load_library(), _lib.ptr, _lib.current_stream()
    n, (h, w) = means.shape[0], depth.shape
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    m_t, w_t, d_t = t(means), t(np.asarray(w2c, F32).reshape(16)), t(depth)
    buf = torch.full((2 * GUARD + ref.VALUES,), FILL, dtype=torch.int64, device=DEV)
    out = buf[GUARD:GUARD + ref.VALUES]
    _lib.check(lib.gsl_map_pose_info(ptr(m_t), n, ptr(w_t), *(float(a) for a in intr), ptr(d_t), w, h, float(keep),
                                     float(beyond), float(kappa), float(near), out.data_ptr(), st), FN)
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + ref.VALUES:] == FILL).all())
    for dev, host in ((m_t, means), (w_t, np.asarray(w2c, F32).reshape(16)), (d_t, depth)):  # the inputs are only read
        assert np.array_equal(dev.cpu().numpy().view(np.uint32), np.ascontiguousarray(host).view(np.uint32))
    return out.cpu().numpy().copy()


# ---- the grid -------------------------------------------------------------------------------------------------------
def _image(name):
    """depth [h,w] float32: 1 / d linear in the pixel on either side of the middle column, another slope on each."""
    w, h = IMAGES[name]
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    left = 0.5 + 0.004 * (u - w / 2.0) + 0.006 * (v - h / 2.0)
    right = 0.5 - 0.012 * (u - w / 2.0) + 0.003 * (v - h / 2.0)
    d = (1.0 / np.where((u < w / 2.0) | (w < 5), left, right)).astype(F32)  # (3x3: its one inner pixel on a plane)
    if name == "33x17":
        d[3, 5], d[7, 20], d[11, 9], d[13, 27] = 0.0, np.nan, np.inf, -1.0
    return d


def _cloud(n, name):
    """means [n,3] float32 in the world of the identity pose (camera = world)."""
    d = _image(name)
    h, w = d.shape
    fx, fy, cx, cy = _intr(w, h)
    rng = np.random.default_rng(1000 * n + w)
    u, v = rng.uniform(-1.0, w, n), rng.uniform(-1.0, h, n)
    at = d[np.clip(np.rint(v), 0, h - 1).astype(int), np.clip(np.rint(u), 0, w - 1).astype(int)].astype(np.float64)
    at = np.where(np.isfinite(at) & (at > 0), at, 2.0)
    z = at * rng.choice([1.0, 1.0, 1.0, 1.003, 0.997, 1.04, 0.96, 1.2, 0.8], n)
    p = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], axis=-1)
    odd = rng.permutation(n)[:n // 16]
    for k, i in enumerate(odd):
        p[i] = [[np.nan, 0.0, 1.0], [0.0, 0.0, -1.0], [0.0, np.inf, 2.0], [0.0, 0.0, np.nan]][k % 4]
    return p.astype(F32)


@pytest.fixture(scope="module")
def clouds():
    return {(n, name): _cloud(n, name) for n in ROWS for name in IMAGES}


@pytest.mark.parametrize("pose", list(POSES))
@pytest.mark.parametrize("name", list(IMAGES))
@pytest.mark.parametrize("n", ROWS)
def test_the_sums_against_the_mirror(n, name, pose, clouds):
    w, h = IMAGES[name]
    depth, means, w2c = _image(name), clouds[(n, name)], ref.w2c_of(POSES[pose])
    want = ref.pose_info(means, w2c, _intr(w, h), depth, KEEP, BEYOND, KAPPA, NEAR)
    if name == "2x2":
        assert not want.any()
    elif n >= 255 and name != "3x3":  # the case is not trivial: rows of every kind
        assert 0 < want[28] < want[29] < n and want[27] > 0 and want[0] > 0, want
    got = _run(means, w2c, _intr(w, h), depth, KEEP, BEYOND, KAPPA, NEAR)
    assert np.array_equal(got, want), (got, want)


def test_two_calls_give_the_same_bits(clouds):
    n, name = ROWS[-1], "33x17"
    args = (clouds[(n, name)], ref.w2c_of(POSES["moved"]), _intr(33, 17), _image(name), KEEP, BEYOND, KAPPA, NEAR)
    first, second = _run(*args), _run(*args)
    assert np.array_equal(first, second) and first[28] > 1000


# ---- the hand-made rows ---------------------------------------------------------------------------------------------
SW, SH = 48, 17
SINTR = _intr(SW, SH)


def _at(u, v, z):
    """The row that projects onto (u, v) at depth z under the identity pose (exact for dyadic u, v, z)."""
    return [(u - SINTR[2]) / 32.0 * z, (v - SINTR[3]) / 32.0 * z, z]


def _specials():
    """(depth [17,48], [(name, row, verdict under kappa = 1, verdict under kappa = 2^-10)]).  Block (bx, by) is the 3x3
    pixels around (3 bx + 2, 3 by + 2); the blocks of by = 0 and by = 4 stay flat."""
    d = np.full((SH, SW), 2.0, F32)
    blocks = iter((bx, by) for by in (1, 2, 3, 4) for bx in range(15))
    cases = []
    side = dict(l=(-1, 0), r=(1, 0), u=(0, -1), d=(0, 1))

    def block(name, z, verdict, flat_verdict, centre=None, all_=None, **nb):
        bx, by = next(blocks)
        cu, cv = 3 * bx + 2, 3 * by + 2
        if all_ is not None:
            d[cv - 1:cv + 2, cu - 1:cu + 2] = all_
        if centre is not None:
            d[cv, cu] = centre
        for k, value in nb.items():
            d[cv + side[k][1], cu + side[k][0]] = value
        cases.append((name, _at(cu, cv, z), verdict, flat_verdict))

    lo, hi = 1.875, 2.125  # 2 * keep, 2 * beyond: exact
    block("on the surface", 2.0, "used", "used")
    block("z == d0 * keep", lo, "used", "used")
    block("a step in front of it", down(lo), "tested", "tested")
    block("z == d0 * beyond", hi, "used", "used")
    block("a step behind it", up(hi), "tested", "tested")
    for k in side:  # a neighbour on the bounds: inside them, and no plane
        block(f"d{k} == d0 * keep", 2.0, "used", "tested", **{k: lo})
        block(f"d{k} a step below", 2.0, "tested", "tested", **{k: down(lo)})
        block(f"d{k} == d0 * beyond", 2.0, "used", "tested", **{k: hi})
        block(f"d{k} a step above", 2.0, "tested", "tested", **{k: up(hi)})
    for k in side:
        for bad in (np.nan, np.inf, 0.0, -1.0):
            block(f"d{k} = {bad}", 2.0, "tested", "tested", **{k: bad})
    for bad in (np.nan, np.inf, 0.0, -1.0):
        block(f"d0 = {bad}", 2.0, "untested", "untested", centre=bad)
    block("z == 64", 64.0, "tested", "tested", all_=64.0)
    block("a step below 64", down(64.0), "used", "used", all_=64.0)
    block("a crease", 2.0, "used", "tested", r=2.1)
    assert len(cases) == 44 and next(blocks)[1] == 3  # the blocks of by = 4 are untouched
    flat = [("z == near", _at(2, 2, NEAR), "untested"), ("a step beyond near", _at(2, 2, up(NEAR)), "tested"),
            ("column 0", _at(0, 2, 2.0), "untested"), ("column 1", _at(1, 2, 2.0), "used"),
            ("column W - 1", _at(SW - 1, 2, 2.0), "untested"), ("column W - 2", _at(SW - 2, 2, 2.0), "used"),
            ("line 0", _at(5, 0, 2.0), "untested"), ("line 1", _at(5, 1, 2.0), "used"),
            ("line H - 1", _at(29, SH - 1, 2.0), "untested"), ("line H - 2", _at(29, SH - 2, 2.0), "used"),
            ("u = 0.5 is column 0", _at(0.5, 2, 2.0), "untested"), ("u = 1.5 is column 2", _at(1.5, 2, 2.0), "used"),
            ("u = W - 1.5 is column W - 2", _at(SW - 1.5, 2, 2.0), "used"),
            ("v = 0.5 is line 0", _at(5, 0.5, 2.0), "untested"), ("v = H - 1.5 is line H - 1", _at(29, SH - 1.5, 2.0), "untested"),
            ("behind the camera", [0.0, 0.0, -2.0], "untested"), ("a NaN row", [np.nan, 0.0, 2.0], "untested"),
            ("a NaN depth", [0.0, 0.0, np.nan], "untested"), ("an inf row", [np.inf, 0.0, 2.0], "untested"),
            ("an inf depth", [0.0, 0.0, np.inf], "untested"), ("outside", _at(-3, 2, 2.0), "untested")]
    cases += [(name, row, verdict, verdict) for name, row, verdict in flat]
    return d, cases


def _verdicts(means, depth, keep, beyond, kappa):
    tested, used, _ = ref.rows(means, np.eye(4, dtype=F32), SINTR, depth, keep, beyond, kappa, NEAR)
    return ["used" if u else "tested" if t else "untested" for t, u in zip(tested, used)]


@pytest.mark.parametrize("kappa", [1.0, 2.0 ** -10])
def test_the_hand_made_rows_are_what_they_say(kappa):
    depth, cases = _specials()
    means = np.array([row for _, row, _, _ in cases], F32)
    want = [big if kappa == 1.0 else small for _, _, big, small in cases]
    got = _verdicts(means, depth, EKEEP, EBEYOND, kappa)
    assert got == want, [(c[0], g, w) for c, g, w in zip(cases, got, want) if g != w]
    # ... and on the device: one row per call is a count of 0 or 1, and the row's own 28 products
    for i, (name, _, _, _) in enumerate(cases):
        sums = _run(means[i:i + 1], np.eye(4, dtype=F32), SINTR, depth, EKEEP, EBEYOND, kappa, NEAR)
        assert sums[28:].tolist() == [int(want[i] == "used"), int(want[i] != "untested")], name
        assert np.array_equal(sums, ref.pose_info(means[i:i + 1], np.eye(4, dtype=F32), SINTR, depth, EKEEP, EBEYOND, kappa,
                                                  NEAR)), name
    all_rows = _run(means, np.eye(4, dtype=F32), SINTR, depth, EKEEP, EBEYOND, kappa, NEAR)
    assert np.array_equal(all_rows, ref.pose_info(means, np.eye(4, dtype=F32), SINTR, depth, EKEEP, EBEYOND, kappa, NEAR))
    assert all_rows[28] == want.count("used") and all_rows[29] == len(want) - want.count("untested")


def test_planarity_at_equality():
    """keep = 0.5, beyond = 2: around d0 = 2 the neighbours 1 and 4 are inside the bounds, on them; 1 / 1 + 1 / 4 misses
    2 / d0 by 1 / 4, which is kappa / d0 at kappa = 0.5."""
    depth = np.full((SH, SW), 2.0, F32)
    depth[5, 4], depth[5, 6] = 1.0, 4.0  # left and right of (5, 5)
    depth[10, 20], depth[12, 20] = 4.0, 1.0  # above and below (20, 11)
    means = np.array([_at(5, 5, 2.0), _at(20, 11, 2.0), _at(12, 8, 2.0)], F32)
    below = float(np.nextafter(F32(0.5), F32(0)))
    assert _verdicts(means, depth, 0.5, 2.0, 0.5) == ["used", "used", "used"]
    assert _verdicts(means, depth, 0.5, 2.0, below) == ["tested", "tested", "used"]
    for kappa, used in ((0.5, 3), (below, 1), (0.0, 1)):
        want = ref.pose_info(means, np.eye(4, dtype=F32), SINTR, depth, 0.5, 2.0, kappa, NEAR)
        assert want[28:].tolist() == [used, 3]
        assert np.array_equal(_run(means, np.eye(4, dtype=F32), SINTR, depth, 0.5, 2.0, kappa, NEAR), want), kappa


# ---- the entry point's refusals, GaussianMap.pose_information -------------------------------------------------------
def test_entry_point_rejects_bad_arguments_without_a_launch(repo_root):
    from tests.test_abi import prototypes

    lib = _lib.load_library()
    params = prototypes(repo_root)[FN][1]
    buffers = {n: torch.full((65536,), 0x7F7F7F7F, dtype=torch.int32, device=DEV)
               for t, n in params if "*" in t and n != "stream"}
    pointers = {n: b.data_ptr() for n, b in buffers.items()}
    for what, over in REFUSED:
        assert call_with(lib, params, dict(GOOD, **over), pointers) == BAD_ARG, what
    torch.cuda.synchronize()
    for name, b in buffers.items():
        assert bool((b == 0x7F7F7F7F).all()), name


def test_pose_information_of_a_map_filled_by_insert_frame():
    w, h = 64, 48
    K = replica_intrinsics(w, h)
    pose = torch.from_numpy(yaw_pose((0.6, 0.1, 0.8), 35.0)).float()
    truth = torch.from_numpy(yaw_pose((0.62, 0.1, 0.79), 36.0)).float()
    depth = room_depth(w, h, K, truth)
    # the pose that is asked about is an estimate, 3 mm and 0.1 degrees off: at the truth itself this noiseless frame
    # leaves residuals below the 2^-10 m that the fixed point of r * r resolves, and sigma would be 0
    query = apply_twist(truth, [0.001, -0.0012, 0.0008, 0.002, -0.001, 0.002])
    rgb = torch.randint(0, 255, (h, w, 3), generator=torch.Generator().manual_seed(3)).float()
    m = GaussianMap(w, h, MapConfig(info=True), DEV)
    empty = m.pose_information(depth, K, query, NEAR)
    assert empty.used == 0 and empty.weak() and m._info is None  # empty: no launch
    assert m.insert_frame(room_depth(w, h, K, pose), rgb, K, pose) == (w * h, w * h)
    before = m.points.clone()
    got = m.pose_information(depth, K, query, NEAR)
    intr = tuple(float(F32(a)) for a in intrinsics(K))
    want = ref.pose_info(m.points.cpu().numpy(), ref.w2c_of(query.numpy()), intr, depth.numpy(), KEEP, BEYOND, KAPPA, NEAR)
    H, g, rss, used, tested = ref.unpack(want)
    assert np.array_equal(got.H, H) and np.array_equal(got.g, g) and (got.rss, got.used, got.tested) == (rss, used, tested)
    assert used > 1000 and rss > 0.0 and not got.weak() and np.all(np.linalg.eigvalsh(got.covariance()) > 0.0)
    assert torch.equal(m.points, before) and m.n_live == w * h and m._info.shape == (30,) and m._info.dtype == torch.int64
    again = m.pose_information(depth, K, query, NEAR)  # the buffer is reused, the sums zeroed again
    assert np.array_equal(again.H, got.H) and np.array_equal(again.g, got.g) and again.rss == got.rss
