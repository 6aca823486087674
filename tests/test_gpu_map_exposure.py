"""GPU: gsl_map_exposure_estimate and gsl_map_exposure_apply (csrc/map_exposure.hip) against the numpy mirror
tests/map_exposure_ref.py on given arrays -- the seven sums of the last pass, the bits of params and every record, bit for
bit -- and GaussianMap.estimate_exposure / apply_exposure.

The grid: the images 3x3, 7x5 and 33x17 and the clouds of tests/test_gpu_map_info.py (depths of 0, NaN, +inf and -1 in
the largest, rows of NaN and inf), the intensities and colours of tests/test_gpu_map_photo.py (NaN, +inf, a step outside
0 .. 1), and a second set of colours that follow the image at the row's pixel (gain 0.9, offset 0.05, noise of +-0.15)
so that the first pass is OK and the gate of the second one cuts; row counts 1, 63 / 64 / 65, 255 / 256 / 257, 1025 and
once one trip of the capped grid plus 1; the identity and a moved pose; 1 and 2 passes.  min_used is 16 there and the
gains 0.25 .. 4.

The hand-made rows (identity pose; fx = fy = 8, cx = 24, cy = 8 on a 48x17 image of depth 2 m; keep = 0.9375, beyond =
1.0625; one row per call, min_used 1, two passes: a single row is FLAT, so params stay (1, 0) and the second record
counts the row behind the gate max_residual; the verdict -- seen, used in the first pass, used in the second -- is
asserted on the mirror first): Y0 and Yi at either end of the saturation range and a float32 step outside; the residual
at the gate and a step above; z at keep * d0 and beyond * d0 and a step outside; depths 0, NaN, +inf, -1; column 0 and
column W - 1, u = -0.5 (rintf gives -0, which is column 0: map_dev.h), u = -0.75 and u = W - 0.5 (outside).

sums, params and record are handed over inside guard words; the inputs are compared bit for bit after the call; two
calls give the same integers; every refusal of tests/test_map_exposure_cpu.py is repeated with device pointers."""
import math
import os
import re

import numpy as np
import pytest
import torch

from gsplatloc_amd import _lib
from gsplatloc_amd.mapping import GaussianMap, MapConfig
from tests import map_exposure_ref as ref
from tests import map_photo_ref as photo
from tests.test_gpu_map_info import CAP, IMAGES, POSES, THREADS, _cloud, _image, _intr
from tests.test_gpu_map_photo import _colors, _intensity
from tests.test_map_exposure_cpu import (ALIGN, BAD_ARG, SH, SINTR, SW, call_with, centre_rows, grey_rows, refusals)

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
NEAR = 0.01
EKEEP, EBEYOND = F32(0.9375), F32(1.0625)
KEEP, BEYOND, KAPPA = photo.keep_of(0.05), photo.beyond_of(0.05), F32(1e-3)
FILL = 0x7F7F7F7F7F7F7F7F
GUARD = 8  # int64 words around sums, params and record
NAMES = ["3x3", "7x5", "33x17"]
ROWS = [1, 63, 64, 65, 255, 256, 257, 1025]
EYE = np.eye(4, dtype=F32)
up, down = (lambda x: float(np.nextafter(F32(x), F32(np.inf)))), (lambda x: float(np.nextafter(F32(x), F32(-np.inf))))
# sat_lo, sat_hi, max_residual, passes, min_used, gain_min, gain_max, offset_max, min_var
GRID = (F32(0.02), F32(0.98), F32(0.1), 2, 16, 0.25, 4.0, 0.5, 1e-4)


def test_the_grid_of_the_kernel_is_the_one_the_row_counts_are_for():
    src = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "map_exposure.hip")).read()
    assert int(re.search(r"constexpr int EXPOSURE_MAX_BLOCKS = (\d+);", src).group(1)) == CAP
    assert int(re.search(r"constexpr int EXPOSURE_THREADS = (\d+);", src).group(1)) == THREADS == 256


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _run(means, colors, w2c, intr, depth, image, keep, beyond, near, sat_lo, sat_hi, rmax, passes, min_used, gain_min,
         gain_max, offset_max, min_var):
    """The entry point on sums, params and record inside guard words: (int64 [7], float32 [4], int64 [passes,6]).  The
    inputs and the guards keep their bits."""
    lib, ptr, st = _lib.load_library(), _lib.ptr, _lib.current_stream()
    n, (h, w) = means.shape[0], depth.shape
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    host = (means, colors, np.asarray(w2c, F32).reshape(16), depth, image)
    m_t, c_t, w_t, d_t, y_t = (t(a) for a in host)
    n_rec = passes * ref.RECORD_WORDS
    at_sums, at_params = GUARD, 2 * GUARD + ref.VALUES
    at_rec = at_params + 2 + GUARD
    buf = torch.full((at_rec + n_rec + GUARD,), FILL, dtype=torch.int64, device=DEV)
    base = buf.data_ptr()
    _lib.check(lib.gsl_map_exposure_estimate(ptr(m_t), ptr(c_t), n, ptr(w_t), *(float(a) for a in intr), ptr(d_t),
                                             ptr(y_t), w, h, float(keep), float(beyond), float(near), float(sat_lo),
                                             float(sat_hi), float(rmax), int(passes), int(min_used), float(gain_min),
                                             float(gain_max), float(offset_max), float(min_var), base + 8 * at_sums,
                                             base + 8 * at_params, base + 8 * at_rec, st), "gsl_map_exposure_estimate")
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    guards = np.concatenate([got[:GUARD], got[at_sums + ref.VALUES:at_params], got[at_params + 2:at_rec],
                             got[at_rec + n_rec:]])
    assert (guards == FILL).all() and len(guards) == 4 * GUARD
    for dev, was in zip((m_t, c_t, w_t, d_t, y_t), host):  # the inputs are only read
        assert np.array_equal(_bits(dev.cpu().numpy()), _bits(was))
    return (got[at_sums:at_sums + ref.VALUES].copy(), got[at_params:at_params + 2].copy().view(F32),
            got[at_rec:at_rec + n_rec].copy().reshape(passes, ref.RECORD_WORDS))


def _same(got, want):
    (sums, params, record), (want_sums, want_params, want_record) = got, want
    assert np.array_equal(sums, want_sums), (sums, want_sums)
    assert np.array_equal(_bits(params), _bits(want_params)), (params, want_params)
    assert np.array_equal(record, ref.record_words(want_record)), (record, want_record)


# ---- the grid -------------------------------------------------------------------------------------------------------
def _matched(n, name):
    """Colours that follow the image: a grey of 0.9 Y + 0.05 at the row's own pixel under the identity pose, noise of
    +-0.15, and the odd colours (NaN, inf, outside 0 .. 1) of tests/test_gpu_map_photo.py."""
    w, h = IMAGES[name]
    means, y = _cloud(n, name), _intensity(name)
    fx, fy, cx, cy = _intr(w, h)
    with np.errstate(all="ignore"):
        u = np.nan_to_num(np.rint(fx * means[:, 0] / means[:, 2] + cx), nan=0.0, posinf=0.0, neginf=0.0)
        v = np.nan_to_num(np.rint(fy * means[:, 1] / means[:, 2] + cy), nan=0.0, posinf=0.0, neginf=0.0)
    at = np.nan_to_num(y[np.clip(v, 0, h - 1).astype(int), np.clip(u, 0, w - 1).astype(int)], nan=0.5, posinf=0.5)
    rng = np.random.default_rng(31 * n + w)
    grey = (0.9 * at + 0.05 + rng.uniform(-0.15, 0.15, n)).astype(F32)
    odd = _colors(n, name)
    c = np.repeat(grey[:, None], 3, axis=1)
    special = ~((odd >= 0.0) & (odd <= 1.0)).all(axis=1)  # NaN, inf, outside 0 .. 1: an eighth of the rows
    c[special] = odd[special]
    return c


@pytest.fixture(scope="module")
def clouds():
    return {(n, name): (_cloud(n, name), _colors(n, name), _matched(n, name)) for n in ROWS for name in NAMES}


@pytest.mark.parametrize("passes", [1, 2])
@pytest.mark.parametrize("pose", list(POSES))
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("n", ROWS)
def test_the_estimate_against_the_mirror(n, name, pose, passes, clouds):
    w, h = IMAGES[name]
    means, random, matched = clouds[(n, name)]
    w2c = photo.w2c_of(POSES[pose])
    params = GRID[:3] + (passes,) + GRID[4:]
    for colors in (random, matched):
        args = (means, colors, w2c, _intr(w, h), _image(name), _intensity(name), KEEP, BEYOND, NEAR) + params
        want = ref.estimate(*args)
        if n >= 255 and name != "3x3":  # the case is not trivial: rows of every kind
            first = want[2][0]
            assert 0 < first[1] < first[2] < n, first
            if colors is matched and pose == "identity":  # the first pass solves, the gate of the second cuts (the moved
                # pose shifts the image under the rows by a quarter of its wavelength: RANGE, which the grid covers so)
                assert first[0] == ref.OK and (passes == 1 or 0 < want[2][1][1] < first[1]), want[2]
        _same(_run(*args), want)


def test_the_capped_grid_plus_one_and_two_calls():
    """The grid-stride loop runs twice for the first row; two calls give the same integers."""
    n, name = CAP * THREADS + 1, "33x17"
    args = (_cloud(n, name), _matched(n, name), photo.w2c_of(POSES["identity"]), _intr(33, 17), _image(name),
            _intensity(name), KEEP, BEYOND, NEAR) + GRID
    want = ref.estimate(*args)
    assert [r[0] for r in want[2]] == [ref.OK, ref.OK] and 1000 < want[2][1][1] < want[2][0][1] < want[2][0][2] < n
    first, second = _run(*args), _run(*args)
    _same(first, want)
    _same(second, want)


# ---- the hand-made rows ---------------------------------------------------------------------------------------------
def _at(u, v, z):
    return [(u - SINTR[2]) / 8.0 * z, (v - SINTR[3]) / 8.0 * z, z]


def _grey_y(c):
    return float((ref.WR * F32(c) + ref.WG * F32(c)) + ref.WB * F32(c))


def _specials():
    """[(name, row, grey, depth, image, sat_lo, sat_hi, max_residual, (seen, used in pass 1, used in pass 2))]."""
    flat = np.full((SH, SW), 2.0, F32)
    cases = []

    def case(name, verdict, at=(24.0, 8.0), z=2.0, grey=0.5, y0=0.5, lo=0.02, hi=0.98, rmax=1.0, d0=2.0):
        depth, image = flat.copy(), np.full((SH, SW), 0.25, F32)
        px = (int(min(max(round(at[0]), 0), SW - 1)), int(at[1]))
        depth[px[1], px[0]], image[px[1], px[0]] = d0, y0
        cases.append((name, _at(at[0], at[1], z), grey, depth, image, lo, hi, rmax, verdict))

    yi = _grey_y(0.3)
    case("Y0 == sat_lo", (1, 1, 1), y0=0.125, lo=0.125)
    case("Y0 a step below sat_lo", (1, 0, 0), y0=down(0.125), lo=0.125)
    case("Y0 == sat_hi", (1, 1, 1), y0=0.75, hi=0.75)
    case("Y0 a step above sat_hi", (1, 0, 0), y0=up(0.75), hi=0.75)
    case("Yi == sat_lo", (1, 1, 1), grey=0.3, lo=yi)
    case("Yi a step below sat_lo", (1, 0, 0), grey=0.3, lo=up(yi))
    case("Yi == sat_hi", (1, 1, 1), grey=0.3, y0=0.25, hi=yi)
    case("Yi a step above sat_hi", (1, 0, 0), grey=0.3, y0=0.25, hi=down(yi))
    rc = float(F32(0.75) - F32(yi))  # params stay (1, 0): (1 * Y0 + 0) - Yi
    case("the residual == max_residual", (1, 1, 1), grey=0.3, y0=0.75, rmax=rc)
    case("the residual a step above the gate", (1, 1, 0), grey=0.3, y0=0.75, rmax=down(rc))
    case("a NaN intensity", (1, 0, 0), y0=np.nan)
    case("an infinite intensity", (1, 0, 0), y0=np.inf)
    case("z == keep * d0", (1, 1, 1), z=1.875)
    case("z a step below keep * d0", (0, 0, 0), z=down(1.875))
    case("z == beyond * d0", (1, 1, 1), z=2.125)
    case("z a step above beyond * d0", (0, 0, 0), z=up(2.125))
    for bad in (0.0, np.nan, np.inf, -1.0):
        case(f"depth {bad}", (0, 0, 0), d0=bad)
    case("column 0", (1, 1, 1), at=(0.0, 8.0))
    case("column W - 1", (1, 1, 1), at=(SW - 1.0, 8.0))
    case("row 0", (1, 1, 1), at=(24.0, 0.0))
    case("row H - 1", (1, 1, 1), at=(24.0, SH - 1.0))
    case("u = -0.5 is column 0 (-0)", (1, 1, 1), at=(-0.5, 8.0))
    case("u = -0.75", (0, 0, 0), at=(-0.75, 8.0))
    case("u = W - 0.5", (0, 0, 0), at=(SW - 0.5, 8.0))
    case("behind the near plane", (0, 0, 0), z=0.005, d0=0.005)
    return cases


def test_the_hand_made_rows_are_what_they_say():
    cases = _specials()
    assert len(cases) == 28
    for name, row, grey, depth, image, lo, hi, rmax, verdict in cases:
        means, colors = np.array([row], F32), np.full((1, 3), grey, F32)
        args = (means, colors, EYE, SINTR, depth, image, EKEEP, EBEYOND, NEAR, F32(lo), F32(hi), F32(rmax), 2, 1, 0.5, 2.0,
                0.25, 1e-4)
        want = ref.estimate(*args)
        rec = want[2]
        assert (rec[0][2], rec[0][1], rec[1][1]) == verdict, (name, rec)
        assert rec[0][0] == (ref.FLAT if verdict[1] else ref.FEW) and np.array_equal(want[1], ref.IDENTITY), (name, rec)
        _same(_run(*args), want)


# ---- the solve ------------------------------------------------------------------------------------------------------
def test_each_status_leaves_the_parameters_of_the_pass_before():
    means, depth = centre_rows()
    colors, yi = grey_rows()
    image = (F32(0.5) * yi + F32(0.125)).astype(F32)
    n = SW * SH
    base = dict(sat_lo=F32(0.02), sat_hi=F32(0.98), max_residual=F32(0.1), passes=2, min_used=256, gain_min=0.5,
                gain_max=4.0, offset_max=0.5, min_var=1e-4)
    identity = _bits(ref.IDENTITY).tolist()
    for what, img, over, statuses in (
            ("used == min_used", image, dict(min_used=n), [ref.OK, ref.OK]),
            ("used == min_used - 1", image, dict(min_used=n + 1), [ref.FEW, ref.FEW]),
            ("a constant image", np.full((SH, SW), 0.5, F32), {}, [ref.FLAT, ref.FLAT]),
            ("a gain just beyond gain_max", image, dict(gain_max=1.999), [ref.RANGE, ref.RANGE]),
            ("an offset beyond offset_max", image, dict(offset_max=0.2), [ref.RANGE, ref.RANGE]),
            ("the second pass is short", (F32(0.51) * yi + F32(0.125)).astype(F32),
             dict(max_residual=F32(0.0), min_used=n // 2), [ref.OK, ref.FEW])):
        p = dict(base, **over)
        args = (means, colors, EYE, SINTR, depth, img, KEEP, BEYOND, NEAR) + tuple(p.values())
        want = ref.estimate(*args)
        assert [r[0] for r in want[2]] == statuses, (what, want[2])
        got = _run(*args)
        _same(got, want)
        if statuses[0] != ref.OK:
            assert _bits(got[1]).tolist() == identity, what
        elif statuses[1] != ref.OK:  # what the first pass left, bit for bit
            one = _run(*(args[:12] + (1,) + args[13:]))
            assert _bits(got[1]).tolist() == _bits(one[1]).tolist() != identity, what


# ---- apply ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(3, 3), (7, 5), (33, 17), (160, 120)])
def test_apply_against_the_mirror(size):
    w, h = size
    rng = np.random.default_rng(w)
    rgb = rng.uniform(-40.0, 300.0, (h, w, 3)).astype(F32)
    rgb[0, 0], rgb[h - 1, w - 1], rgb[1, 1], rgb[1, 2] = (0.0, 255.0, 127.5), (255.0, 0.0, 1e-3), (np.nan, np.inf, -np.inf), (
        17.904108 / 1.1755924, 300.0, -1.0)
    rgb[0, 1] = (-40.0, 300.0, 255.0)  # clip at both ends under every pair below
    lib, ptr, st = _lib.load_library(), _lib.ptr, _lib.current_stream()
    for params in (ref.params_of(1.1755924, -0.07021219), ref.params_of(0.8, 0.06), ref.IDENTITY):
        rgb_t, p_t = torch.from_numpy(rgb).to(DEV), torch.from_numpy(params).to(DEV)
        buf = torch.full((h * w * 3 + 2 * GUARD,), -7.0, device=DEV)
        _lib.check(lib.gsl_map_exposure_apply(ptr(rgb_t), w, h, ptr(p_t), buf[GUARD:].data_ptr(), st),
                   "gsl_map_exposure_apply")
        torch.cuda.synchronize()
        got = buf[GUARD:GUARD + h * w * 3].cpu().numpy().reshape(h, w, 3)
        want = ref.apply(rgb, params)
        assert np.array_equal(_bits(got), _bits(want))
        assert np.isnan(got[1, 1, 0]) and got[1, 1, 1] == 255.0 and got[1, 1, 2] == 0.0 and np.nanmin(got) >= 0.0 and np.nanmax(got) <= 255.0
        assert (want == 0.0).sum() > 1 and (want == 255.0).sum() > 1  # both ends clip
        assert bool((buf[:GUARD] == -7.0).all()) and bool((buf[GUARD + h * w * 3:] == -7.0).all())
        assert np.array_equal(_bits(rgb_t.cpu().numpy()), _bits(rgb)) and np.array_equal(_bits(p_t.cpu().numpy()), _bits(params))
        m = GaussianMap(w, h, MapConfig(), DEV)
        if params is ref.IDENTITY:
            assert np.array_equal(_bits(m.apply_exposure(torch.from_numpy(rgb)).cpu().numpy()), _bits(want))
        assert np.array_equal(_bits(m.apply_exposure(torch.from_numpy(rgb), (params[0], params[1])).cpu().numpy()), _bits(want))


# ---- the refusals, with device pointers -----------------------------------------------------------------------------
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


# ---- through GaussianMap: the wall under another exposure -----------------------------------------------------------
def test_the_wall_through_the_map():
    """estimate_exposure equals the mirror; apply_exposure followed by align_pose(intensity=) ends at the mirror's pose
    bit for bit; an empty map launches nothing."""
    c = photo.wall_case()
    w, h = photo.WALL_W, photo.WALL_H
    fx, fy, cx, cy = photo.WALL_INTR
    K = torch.tensor([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
    raw = (F32(0.85) * c["rgb"] + F32(255.0 * 0.06)).astype(F32)
    depth_t, raw_t = torch.from_numpy(c["depth"]), torch.from_numpy(raw)
    m = GaussianMap(w, h, MapConfig(align=True, photo_scale=0.2, photo_max_residual=0.1, photo_exposure=True), DEV)
    empty = m.estimate_exposure(depth_t, K, torch.eye(4), NEAR, rgb=raw_t)
    assert (empty.gain, empty.offset, empty.status, empty.used) == (1.0, 0.0, "FEW", 0) and m._exposure is None
    d0, rgb0 = photo.wall_frame(np.eye(4))
    assert m.insert_frame(torch.from_numpy(d0), torch.from_numpy(rgb0), K, torch.eye(4)) == (w * h, w * h)
    means, colors = m.points.cpu().numpy(), m.point_colors.cpu().numpy()
    image = photo.intensity(raw)
    want_sums, want_params, want_record = ref.estimate(means, colors, EYE, c["intr"], c["depth"], image, KEEP, BEYOND, NEAR,
                                                       *ref.DEFAULTS)
    got = m.estimate_exposure(depth_t, K, torch.eye(4), NEAR, rgb=raw_t)
    assert got.ok and (F32(got.gain), F32(got.offset)) == (want_params[0], want_params[1])
    assert got.history == [(ref.NAMES[r[0]],) + tuple(r[1:]) for r in want_record]
    assert (got.used, got.seen, got.rss) == (want_record[-1][1], want_record[-1][2], want_record[-1][5])
    assert abs(got.gain - 1.0 / 0.85) <= 2e-3 and abs(got.offset + 0.06 / 0.85) <= 1e-3
    same = m.estimate_exposure(depth_t, K, torch.eye(4), NEAR, intensity=m.intensity(raw_t))
    assert same == got
    # the device's pair, a given Exposure and a given pair correct alike
    fixed = m.apply_exposure(raw_t)
    want_fixed = ref.apply(raw, want_params)
    assert np.array_equal(_bits(fixed.cpu().numpy()), _bits(want_fixed))
    assert torch.equal(m.apply_exposure(raw_t, got), fixed) and torch.equal(m.apply_exposure(raw_t, (got.gain, got.offset)), fixed)
    before = m.points.clone()
    al = m.align_pose(depth_t, K, torch.eye(4), NEAR, intensity=m.intensity(fixed))
    P = photo.pose_align(means, colors, EYE, c["intr"], c["depth"], photo.intensity(want_fixed), KEEP, BEYOND, KAPPA, NEAR,
                         0.2, 0.1, *ALIGN)[0]
    assert np.array_equal(al.w2c64[:3].view(np.uint64), P.view(np.uint64)) and al.status == "CONVERGED"
    off = m.align_pose(depth_t, K, torch.eye(4), NEAR, intensity=m.intensity(raw_t))
    e_fixed, e_off = photo.pose_error(al.w2c64, c["truth"])[0], photo.pose_error(off.w2c64, c["truth"])[0]
    assert e_fixed <= 0.1 * e_off and torch.equal(m.points, before), (e_fixed, e_off)
    assert math.isclose(float(m.intensity(fixed).mean()), float(c["image"].mean()), abs_tol=2e-3)
