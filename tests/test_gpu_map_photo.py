"""GPU: gsl_map_photo_intensity and gsl_map_pose_info_photo (csrc/map_photo.hip) against the numpy mirror
tests/map_photo_ref.py on given arrays -- the intensity image, all 30 integers and the two extra words, bit for bit --
and GaussianMap.intensity / pose_information(intensity=).

The grid: the images 3x3 (one inner pixel), 7x5 and 33x17 of tests/test_gpu_map_info.py -- two planes that meet in a
crease, the largest with pixels of depth 0, NaN, +inf and -1 -- with an intensity image that is smooth but for pixels of
NaN, +inf, a step below 0 and a step above 1 stamped into the largest; the clouds of that file with a colour per row,
uniform in 0 .. 1 but for every 16th, which is NaN, +inf, below 0 or above 1 in a channel, and as many greys one step
outside 0 .. 1; row counts 1, 63 / 64 / 65, 255 / 256 /
257, 1025, and once one trip of the capped grid plus 1; the identity and a moved pose.  photo_max_residual is 0.5 there,
so that a random colour passes the gate or does not in comparable numbers.

The hand-made rows (identity pose; fx = fy = 8, cx = 24, cy = 8 on a 48x17 image of depth 2 m, so that a row on a pixel
centre has dyadic coordinates and a wide enough angle to reach the gate on a2; keep = 0.9375, beyond = 1.0625; one row
per call, its verdict asserted on the mirror first):
  |rc| equal to photo_max_residual and the gate one float32 step below |rc|;
  a0 = (s gx) fx / z = 8 with gx = 1/2, s = 4 -- taken -- and s one step above -- not; a1 likewise with gy; a2 =
  -(a0 x) / z = -8 at x = 2 z with s = 2, and one step above;
  z == 16 on a surface at 16 m -- geometry only -- and one step below -- both;
  each of the five intensities in turn NaN, +inf, one step below 0 and one step above 1, and a row colour that is NaN or
  +inf in one channel, or a grey one step below 0 or one step above 1 in every channel (the rule tests the weighted sum
  Yi, which is then one step outside as well: the product of 0.587f and the smallest subnormal rounds back to it):
  geometry only, ``used`` unchanged; one channel alone a step above 1 leaves Yi inside: both.
A constant image gives every used row an equation whose only non-zero product is (s rc)^2; photo_scale = 0 gives
gsl_map_pose_info's integers on the same buffers.

out and extra are handed over inside guard words; the inputs are compared bit for bit after the call; two calls give the
same integers; every refusal of tests/test_map_photo_cpu.py is repeated with device pointers: nothing is written."""
import numpy as np
import pytest
import torch

from gsplatloc_amd import _lib
from gsplatloc_amd.mapping import GaussianMap, MapConfig, apply_twist
from gsplatloc_amd.synthetic import replica_intrinsics, room_depth
from tests import map_info_ref as info
from tests import map_photo_ref as ref
from tests.test_gpu_map_info import CAP, IMAGES, POSES, THREADS, _cloud, _image, _intr
from tests.test_map_info_cpu import intrinsics, yaw_pose
from tests.test_map_photo_cpu import BAD_ARG, call_with, refusals

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
NEAR = 0.01
EKEEP, EBEYOND = F32(0.9375), F32(1.0625)
KEEP, BEYOND, KAPPA = ref.keep_of(0.05), ref.beyond_of(0.05), F32(1e-3)
FILL = 0x7F7F7F7F7F7F7F7F
GUARD = 8  # int64 words on either side of out and of extra
NAMES = ["3x3", "7x5", "33x17"]
ROWS = [1, 63, 64, 65, 255, 256, 257, 1025]
up, down = (lambda x: float(np.nextafter(F32(x), F32(np.inf)))), (lambda x: float(np.nextafter(F32(x), F32(-np.inf))))
BELOW_0, ABOVE_1 = down(0.0), up(1.0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _run(means, colors, w2c, intr, depth, image, keep, beyond, kappa, near, scale, rmax):
    """The entry point on out and extra inside guard words: (int64 [30], int64 [2]).  The inputs and the guards keep
    their bits."""
    lib, ptr, st = _lib.load_library(), _lib.ptr, _lib.current_stream()
    n, (h, w) = means.shape[0], depth.shape
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    host = (means, colors, np.asarray(w2c, F32).reshape(16), depth, image)
    m_t, c_t, w_t, d_t, y_t = (t(a) for a in host)
    buf = torch.full((3 * GUARD + ref.VALUES + 2,), FILL, dtype=torch.int64, device=DEV)
    out, extra = buf[GUARD:GUARD + ref.VALUES], buf[2 * GUARD + ref.VALUES:2 * GUARD + ref.VALUES + 2]
    _lib.check(lib.gsl_map_pose_info_photo(ptr(m_t), n, ptr(w_t), *(float(a) for a in intr), ptr(d_t), w, h, float(keep),
                                           float(beyond), float(kappa), float(near), out.data_ptr(), ptr(c_t), ptr(y_t),
                                           float(scale), float(rmax), extra.data_ptr(), st), "gsl_map_pose_info_photo")
    torch.cuda.synchronize()
    guards = torch.cat([buf[:GUARD], buf[GUARD + ref.VALUES:2 * GUARD + ref.VALUES], buf[2 * GUARD + ref.VALUES + 2:]])
    assert bool((guards == FILL).all())
    for dev, was in zip((m_t, c_t, w_t, d_t, y_t), host):  # the inputs are only read
        assert np.array_equal(_bits(dev.cpu().numpy()), _bits(was))
    return out.cpu().numpy().copy(), extra.cpu().numpy().copy()


# ---- the intensity image --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(3, 3), (7, 5), (33, 17), (160, 120)])
def test_the_intensity_image_against_the_mirror(size):
    w, h = size
    rng = np.random.default_rng(w)
    rgb = rng.uniform(0.0, 255.0, (h, w, 3)).astype(F32)
    rgb[0, 0], rgb[h - 1, w - 1], rgb[1, 1] = (0.0, 0.0, 0.0), (255.0, 255.0, 255.0), (np.nan, 1.0, np.inf)
    lib, ptr, st = _lib.load_library(), _lib.ptr, _lib.current_stream()
    rgb_t = torch.from_numpy(rgb).to(DEV)
    buf = torch.full((h * w + 2 * GUARD,), -7.0, device=DEV)
    _lib.check(lib.gsl_map_photo_intensity(ptr(rgb_t), w, h, buf[GUARD:].data_ptr(), st), "gsl_map_photo_intensity")
    torch.cuda.synchronize()
    got = buf[GUARD:GUARD + h * w].cpu().numpy().reshape(h, w)
    assert np.array_equal(_bits(got), _bits(ref.intensity(rgb)))
    assert bool((buf[:GUARD] == -7.0).all()) and bool((buf[GUARD + h * w:] == -7.0).all())
    assert np.array_equal(_bits(rgb_t.cpu().numpy()), _bits(rgb))
    m = GaussianMap(w, h, MapConfig(), DEV)
    assert np.array_equal(_bits(m.intensity(torch.from_numpy(rgb)).cpu().numpy()), _bits(got))


# ---- the grid -------------------------------------------------------------------------------------------------------
def _intensity(name):
    """[h,w] float32 in 0.2 .. 0.8, smooth; the largest with pixels no equation may read."""
    w, h = IMAGES[name]
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    y = (0.5 + 0.2 * np.sin(0.9 * u + 0.3 * v) + 0.1 * np.cos(0.7 * v - 0.2 * u)).astype(F32)
    if name == "33x17":
        y[4, 9], y[8, 22], y[12, 5], y[6, 28] = np.nan, np.inf, BELOW_0, ABOVE_1
    return y


def _colors(n, name):
    rng = np.random.default_rng(77 * n + IMAGES[name][0])
    c = rng.uniform(0.0, 1.0, (n, 3)).astype(F32)
    for k, i in enumerate(rng.permutation(n)[:n // 16]):
        c[i, k % 3] = [np.nan, np.inf, -0.25, 1.5][k % 4]
    for k, i in enumerate(rng.permutation(n)[:n // 16]):  # greys a step outside 0 .. 1: Yi is a step outside too
        c[i] = [BELOW_0, ABOVE_1][k % 2]
    return c


@pytest.fixture(scope="module")
def clouds():
    return {(n, name): (_cloud(n, name), _colors(n, name)) for n in ROWS for name in NAMES}


@pytest.mark.parametrize("pose", list(POSES))
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("n", ROWS)
def test_the_sums_against_the_mirror(n, name, pose, clouds):
    w, h = IMAGES[name]
    (means, colors), w2c = clouds[(n, name)], ref.w2c_of(POSES[pose])
    args = (means, colors, w2c, _intr(w, h), _image(name), _intensity(name), KEEP, BEYOND, KAPPA, NEAR, 0.2, 0.5)
    want, want_extra = ref.pose_info(*args)
    if n >= 255 and name != "3x3":  # the case is not trivial: rows of every kind
        assert 0 < want_extra[0] <= want[28] < want[29] < n and want_extra[1] > 0, (want, want_extra)
        geo = info.pose_info(means, w2c, _intr(w, h), _image(name), KEEP, BEYOND, KAPPA, NEAR)
        assert np.array_equal(geo[28:], want[28:]) and (geo[:28] != want[:28]).sum() > 20
    got, got_extra = _run(*args)
    assert np.array_equal(got, want) and np.array_equal(got_extra, want_extra), (got, want, got_extra, want_extra)


def test_the_capped_grid_plus_one_and_two_calls():
    """The grid-stride loop runs twice for the first row; two calls give the same integers."""
    n, name = CAP * THREADS + 1, "33x17"
    assert THREADS == 256
    args = (_cloud(n, name), _colors(n, name), ref.w2c_of(POSES["moved"]), _intr(33, 17), _image(name), _intensity(name),
            KEEP, BEYOND, KAPPA, NEAR, 0.2, 0.5)
    want, want_extra = ref.pose_info(*args)
    first, second = _run(*args), _run(*args)
    assert 1000 < want_extra[0] < want[28]
    for got, got_extra in (first, second):
        assert np.array_equal(got, want) and np.array_equal(got_extra, want_extra)


# ---- the hand-made rows ---------------------------------------------------------------------------------------------
SW, SH = 48, 17
SINTR = (8.0, 8.0, 24.0, 8.0)
EYE = np.eye(4, dtype=F32)


def _at(u, v, z):
    """The row that projects onto (u, v) at depth z under the identity pose (exact for dyadic z)."""
    return [(u - SINTR[2]) / 8.0 * z, (v - SINTR[3]) / 8.0 * z, z]


def _verdict(means, colors, depth, image, scale, rmax):
    _, used, _, photo, _ = ref.rows(means, colors, EYE, SINTR, depth, image, EKEEP, EBEYOND, 1.0, NEAR, scale, rmax)
    return ["both" if p else "geometry" if u else "none" for u, p in zip(used, photo)]


def _specials():
    """[(name, row, colour, depth, image, scale, photo_max_residual, verdict)]."""
    flat, grey = np.full((SH, SW), 2.0, F32), np.full((SH, SW), 0.5, F32)
    cases = []

    def case(name, verdict, at=(24, 8), z=2.0, colour=(0.5, 0.5, 0.5), scale=1.0, rmax=1.0, depth=None, **pixels):
        image = grey.copy()
        side = dict(c=(0, 0), l=(-1, 0), r=(1, 0), u=(0, -1), d=(0, 1))
        for k, value in pixels.items():
            image[at[1] + side[k][1], at[0] + side[k][0]] = value
        cases.append((name, _at(at[0], at[1], z), colour, flat if depth is None else depth, image, scale, rmax, verdict))

    # |rc|: the row sits on its pixel's centre, Yp = Y0 = 0.75 and rc = Y0 - Yi, whatever float32 makes of Yi
    yi = (ref.WR * F32(0.3) + ref.WG * F32(0.3)) + ref.WB * F32(0.3)
    rc = float(F32(0.75) - yi)
    assert 0.4 < rc < 0.5
    case("|rc| == photo_max_residual", "both", colour=(0.3, 0.3, 0.3), rmax=rc, c=0.75)
    case("the gate a step below |rc|", "geometry", colour=(0.3, 0.3, 0.3), rmax=down(rc), c=0.75)
    case("rc == -photo_max_residual", "both", colour=(0.0, 0.0, 0.0), rmax=0.25, c=0.25)  # Yi = 0 exactly
    case("|rc| a step above the gate", "geometry", colour=(0.0, 0.0, 0.0), rmax=0.25, c=up(0.25))
    # a0 = (s * 1/2) * 8 / 2 = 2 s at x = y = 0 (a2 = 0); a1 likewise
    case("a0 == 8", "both", scale=4.0, l=0.0, r=1.0)
    case("a0 a step above 8", "geometry", scale=up(4.0), l=0.0, r=1.0)
    case("a0 == -8", "both", scale=4.0, l=1.0, r=0.0)
    case("a1 == 8", "both", scale=4.0, u=0.0, d=1.0)
    case("a1 a step above 8", "geometry", scale=up(4.0), u=0.0, d=1.0)
    case("a1 == -8", "both", scale=4.0, u=1.0, d=0.0)
    # a2 = -(a0 x) / z at u = 40: x = 2 z = 4, a0 = 2 s = 4, a2 = -8
    case("a2 == -8", "both", at=(40, 8), scale=2.0, l=0.0, r=1.0)
    case("a2 a step beyond -8", "geometry", at=(40, 8), scale=up(2.0), l=0.0, r=1.0)
    case("a2 == 8", "both", at=(8, 8), scale=2.0, l=0.0, r=1.0)
    far = np.full((SH, SW), 16.0, F32)
    case("z == 16", "geometry", z=16.0, depth=far)
    case("z a step below 16", "both", z=down(16.0), depth=far)
    for k in "clrud":
        for bad in (np.nan, np.inf, BELOW_0, ABOVE_1):
            case(f"Y{k} = {bad}", "geometry", **{k: bad})
        case(f"Y{k} = 0", "both", **{k: 0.0})
        case(f"Y{k} = 1", "both", **{k: 1.0})
    for bad in (np.nan, np.inf):
        for ch in range(3):
            colour = [0.5, 0.5, 0.5]
            colour[ch] = bad
            case(f"colour[{ch}] = {bad}", "geometry", colour=tuple(colour))
    # what is tested is Yi, the weighted sum: a grey one step outside in every channel leaves it one step outside --
    # 0.587f times the smallest subnormal rounds back to it, and the three weights of a step above 1 sum to a step above 1
    for bad in (BELOW_0, ABOVE_1, -1e-6, 1.001):
        case(f"a grey of {bad}", "geometry", colour=(bad, bad, bad))
    for ch in range(3):  # one channel a step outside: the sum stays inside
        colour = [0.5, 0.5, 0.5]
        colour[ch] = ABOVE_1
        case(f"colour[{ch}] a step above 1", "both", colour=tuple(colour))
    case("a black row", "both", colour=(0.0, 0.0, 0.0))
    case("a white row under a white image", "both", colour=(1.0, 1.0, 1.0), c=1.0, l=1.0, r=1.0, u=1.0, d=1.0)
    case("a row off the surface", "none", z=3.0)
    return cases


def test_the_hand_made_rows_are_what_they_say():
    cases = _specials()
    assert len(cases) == 61
    for name, row, colour, depth, image, scale, rmax, verdict in cases:
        means, colors = np.array([row], F32), np.array([colour], F32)
        assert _verdict(means, colors, depth, image, scale, rmax) == [verdict], name
        want, want_extra = ref.pose_info(means, colors, EYE, SINTR, depth, image, EKEEP, EBEYOND, 1.0, NEAR, scale, rmax)
        assert [int(want[28]), int(want_extra[0])] == [int(verdict != "none"), int(verdict == "both")], name
        got, got_extra = _run(means, colors, EYE, SINTR, depth, image, EKEEP, EBEYOND, 1.0, NEAR, scale, rmax)
        assert np.array_equal(got, want) and np.array_equal(got_extra, want_extra), (name, got, want, got_extra, want_extra)
        if verdict == "geometry":  # the geometric integers and nothing else
            assert np.array_equal(got, info.pose_info(means, EYE, SINTR, depth, EKEEP, EBEYOND, 1.0, NEAR)), name
    # the gates were reached: the products at them are what the rule says
    by_name = {c[0]: c for c in cases}
    for name, slot, value in (("a0 == 8", (3, 3), 64), ("a1 == -8", (4, 4), 64), ("a2 == -8", (5, 5), 64)):
        _, row, colour, depth, image, scale, rmax, _ = by_name[name]
        both, _ = ref.pose_info(np.array([row], F32), np.array([colour], F32), EYE, SINTR, depth, image, EKEEP, EBEYOND,
                                1.0, NEAR, scale, rmax)
        geo = info.pose_info(np.array([row], F32), EYE, SINTR, depth, EKEEP, EBEYOND, 1.0, NEAR)
        at = ref.SLOTS.index(slot)
        assert both[at] - geo[at] == value << 20, name


def _wall_rows():
    """A flat surface and rows on every inner pixel's centre, grey 0.25."""
    depth = np.full((SH, SW), 2.0, F32)
    means = np.array([_at(u, v, 2.0) for v in range(SH) for u in range(SW)], F32)
    return depth, means, np.full((len(means), 3), 0.25, F32)


def test_a_constant_image_adds_its_residual_and_nothing_else():
    depth, means, colors = _wall_rows()
    image = np.full((SH, SW), 0.5, F32)
    geo = info.pose_info(means, EYE, SINTR, depth, EKEEP, EBEYOND, 1.0, NEAR)
    got, extra = _run(means, colors, EYE, SINTR, depth, image, EKEEP, EBEYOND, 1.0, NEAR, 2.0, 1.0)
    inner = (SW - 2) * (SH - 2)
    assert geo[28] == inner and extra[0] == inner  # every used row counts
    assert np.array_equal(got[:27], geo[:27]) and np.array_equal(got[28:], geo[28:])  # a = 0: the geometric sums
    yi = (ref.WR * F32(0.25) + ref.WG * F32(0.25)) + ref.WB * F32(0.25)
    each = F32(2.0) * (F32(0.5) - yi)
    assert extra[1] == inner * int(np.rint((each * each) * F32(2.0 ** 20))) and got[27] == geo[27] + extra[1]
    want, want_extra = ref.pose_info(means, colors, EYE, SINTR, depth, image, EKEEP, EBEYOND, 1.0, NEAR, 2.0, 1.0)
    assert np.array_equal(got, want) and np.array_equal(extra, want_extra)


@pytest.mark.parametrize("name", NAMES)
def test_scale_zero_is_the_geometric_entry_point_on_the_same_buffers(name):
    w, h = IMAGES[name]
    n = 1025
    means, colors, depth, image = _cloud(n, name), _colors(n, name), _image(name), _intensity(name)
    lib, ptr, st = _lib.load_library(), _lib.ptr, _lib.current_stream()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    m_t, c_t, d_t, y_t = t(means), t(colors), t(depth), t(image)
    w_t = t(ref.w2c_of(POSES["moved"]).reshape(16))
    out = torch.full((2, ref.VALUES + 2), FILL, dtype=torch.int64, device=DEV)
    args = (ptr(m_t), n, ptr(w_t), *_intr(w, h), ptr(d_t), w, h, float(KEEP), float(BEYOND), float(KAPPA), NEAR)
    _lib.check(lib.gsl_map_pose_info(*args, out[0].data_ptr(), st), "gsl_map_pose_info")
    _lib.check(lib.gsl_map_pose_info_photo(*args, out[1].data_ptr(), ptr(c_t), ptr(y_t), 0.0, 0.5,
                                           out[1, ref.VALUES:].data_ptr(), st), "gsl_map_pose_info_photo")
    host = out.cpu().numpy()
    assert np.array_equal(host[0, :ref.VALUES], host[1, :ref.VALUES]) and host[0, 28] > 0
    assert host[0, ref.VALUES:].tolist() == [FILL, FILL] and 0 < host[1, ref.VALUES] <= host[0, 28] and host[1, 31] == 0


# ---- the entry points' refusals, GaussianMap.pose_information ------------------------------------------------------
def test_entry_points_reject_bad_arguments_without_a_launch(repo_root):
    from tests.test_abi import prototypes

    lib, protos = _lib.load_library(), prototypes(repo_root)
    names = {n for fn, _, _ in refusals() for t, n in protos[fn][1] if "*" in t and n != "stream"}
    buffers = {n: torch.full((65536,), 0x7F7F7F7F, dtype=torch.int32, device=DEV) for n in names}
    pointers = {n: b.data_ptr() for n, b in buffers.items()}
    for fn, what, named in refusals():
        assert call_with(lib, fn, protos[fn][1], named, pointers) == BAD_ARG, (fn, what)
    torch.cuda.synchronize()
    for name, b in buffers.items():
        assert bool((b == 0x7F7F7F7F).all()), name


def test_pose_information_of_a_map_filled_by_insert_frame():
    w, h = 64, 48
    K = replica_intrinsics(w, h)
    pose = torch.from_numpy(yaw_pose((0.6, 0.1, 0.8), 35.0)).float()
    truth = torch.from_numpy(yaw_pose((0.62, 0.1, 0.79), 36.0)).float()
    depth = room_depth(w, h, K, truth)
    query = apply_twist(truth, [0.001, -0.0012, 0.0008, 0.002, -0.001, 0.002])
    v, u = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    smooth = 127.5 + 60.0 * torch.sin(0.3 * u + 0.2 * v)
    rgb = torch.stack([smooth, 0.9 * smooth, 0.8 * smooth + 20.0], -1).float()
    m = GaussianMap(w, h, MapConfig(info=True, photo_scale=0.2, photo_max_residual=0.5), DEV)
    image = m.intensity(rgb)
    assert image.shape == (h, w) and image.dtype == torch.float32 and image.is_cuda
    assert np.array_equal(_bits(image.cpu().numpy()), _bits(ref.intensity(rgb.numpy())))
    empty = m.pose_information(depth, K, query, NEAR, intensity=image)
    assert empty.used == 0 and empty.weak() and m._info_photo is None and m._info is None  # empty: no launch
    assert m.insert_frame(room_depth(w, h, K, pose), rgb, K, pose) == (w * h, w * h)
    before = m.points.clone()
    got = m.pose_information(depth, K, query, NEAR, intensity=image)
    intr = tuple(float(F32(a)) for a in intrinsics(K))
    want, extra = ref.pose_info(m.points.cpu().numpy(), m.point_colors.cpu().numpy(), ref.w2c_of(query.numpy()), intr,
                                depth.numpy(), image.cpu().numpy(), KEEP, BEYOND, KAPPA, NEAR, 0.2, 0.5)
    H, g, rss, used, tested = ref.unpack(want)
    assert np.array_equal(got.H, H) and np.array_equal(got.g, g) and (got.rss, got.used, got.tested) == (rss, used, tested)
    assert (got.photo_used, got.photo_rss) == (int(extra[0]), float(extra[1]) / 2.0 ** 20) and 1000 < got.photo_used <= used
    assert torch.equal(m.points, before) and m._info is None and m._info_photo.shape == (32,)
    # the call's own scale and gate win over the configuration's; without an image the call is the one of before
    other = m.pose_information(depth, K, query, NEAR, intensity=image, photo_scale=1.0, photo_max_residual=0.05)
    want, extra = ref.pose_info(m.points.cpu().numpy(), m.point_colors.cpu().numpy(), ref.w2c_of(query.numpy()), intr,
                                depth.numpy(), image.cpu().numpy(), KEEP, BEYOND, KAPPA, NEAR, 1.0, 0.05)
    assert np.array_equal(other.H, ref.unpack(want)[0]) and other.photo_used == int(extra[0]) < got.photo_used
    plain = m.pose_information(depth, K, query, NEAR)
    geo = info.pose_info(m.points.cpu().numpy(), ref.w2c_of(query.numpy()), intr, depth.numpy(), KEEP, BEYOND, KAPPA, NEAR)
    assert np.array_equal(plain.H, info.unpack(geo)[0]) and plain.photo_used == 0 and m._info.shape == (30,)
