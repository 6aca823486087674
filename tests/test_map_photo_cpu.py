"""The photometric term of the pose normal equations (csrc/map_photo.hip, MapConfig.photo_scale), the parts that need
no GPU: the numpy mirror tests/map_photo_ref.py against tests/map_info_ref.py at photo_scale = 0; the textured wall,
which depth alone leaves open in three directions and colour closes; the gradient of the summed cost by central
differences; the entry points against their prototypes and every refusal, with host pointers; the row bound; MapConfig
and the host layer's own checks.

The wall (tests/map_photo_ref.py: 160x120, fx = fy = 80, the plane z = 2 m -- or z = 2 + 0.3 x -- whose colour is a
smooth function of the world point; the map is frame 0 back-projected, the query is 0.3 degrees about the optical axis
and (12, -8, 0) mm away, the start is the old pose; rho 0.05, kappa 1e-3, damping 1e-3, 8 steps, the default stop
tolerances).  The float64 prototype of this set-up ended at 1.9e-5 m / 2.2e-4 degrees on the fronto-parallel wall and
at 2.2e-5 m on the slanted one with photo_scale = 0.2 -- the floor of a central-difference gradient and a linear
sub-pixel model -- and that floor is the yardstick.  The float32 mirror measured 1.70e-5 m / 2.10e-4 degrees
(CONVERGED, 4 steps) and 2.25e-5 m / 2.38e-4 degrees (CONVERGED, 5 steps); it differs from the prototype only by the
rounding order of the rule, and the tests assert twice those figures.  What the mirror measures is printed (NOTES.md,
"Photometric term")."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from gsplatloc_amd import _lib, mapping
from gsplatloc_amd.mapping import GaussianMap, MapConfig, PoseInformation, information_from_sums
from gsplatloc_amd.synthetic import replica_intrinsics
from tests import map_align_ref as align
from tests import map_info_ref as info
from tests import map_photo_ref as ref
from tests import test_map_info_cpu as base
from tests.test_abi import prototypes
from tests.test_kernel_resources import HIPCC, _resources

F32 = np.float32
NEAR = 0.01
KEEP, BEYOND, KAPPA = ref.keep_of(0.05), ref.beyond_of(0.05), F32(1e-3)
SCALE, RMAX = 0.2, 0.1
ALIGN = (8, 1e-3, 7, math.radians(12.8), 0.32, math.radians(1.5e-4), 3e-5)  # MapConfig's defaults
# twice what the float32 mirror measured, per wall: (metres, degrees)
WALL_BOUND = {0.0: (2 * 1.70e-5, 2 * 2.10e-4), 0.3: (2 * 2.25e-5, 2 * 2.38e-4)}


# ---- (a) photo_scale = 0 is the geometric rule ----------------------------------------------------------------------
corner = base.corner  # the fixture of tests/test_map_info_cpu.py: the corner view and its three twists


def _grey(n, seed):
    return np.random.default_rng(seed).uniform(0.0, 1.0, (n, 3)).astype(F32)


def test_scale_zero_gives_the_geometric_integers_in_the_corner(corner):
    c = corner
    rng = np.random.default_rng(5)
    image = rng.uniform(0.0, 1.0, c["depth"].shape).astype(F32)
    colors = _grey(len(c["means"]), 6)
    for xi in c["twists"]:
        est = mapping.apply_twist(torch.from_numpy(c["truth"]), xi).numpy()
        w2c = ref.w2c_of(est)
        want = info.pose_info(c["means"], w2c, c["intr"], c["depth"], KEEP, BEYOND, KAPPA, NEAR)
        got, extra = ref.pose_info(c["means"], colors, w2c, c["intr"], c["depth"], image, KEEP, BEYOND, KAPPA, NEAR, 0.0,
                                   1.0)
        assert np.array_equal(got, want) and want[28] > 16000
        # nearly every used row gave an equation, of zeros (the random image throws a few residuals past 1)
        assert 0.99 * want[28] < extra[0] <= want[28] and extra[1] == 0
        some, _ = ref.pose_info(c["means"], colors, w2c, c["intr"], c["depth"], image, KEEP, BEYOND, KAPPA, NEAR, 0.5, 1.0)
        assert not np.array_equal(some[:28], want[:28]) and np.array_equal(some[28:], want[28:])


def test_scale_zero_gives_the_geometric_integers_on_a_plane():
    depth, means = base.plane_case()
    image = np.random.default_rng(7).uniform(0.0, 1.0, depth.shape).astype(F32)
    want = info.pose_info(means, np.eye(4, dtype=F32), base.PINTR, depth, KEEP, BEYOND, KAPPA, NEAR)
    got, extra = ref.pose_info(means, _grey(len(means), 8), np.eye(4, dtype=F32), base.PINTR, depth, image, KEEP, BEYOND,
                               KAPPA, NEAR, 0.0, 1.0)
    assert np.array_equal(got, want) and 0 < extra[0] <= (base.PW - 2) * (base.PH - 2) and extra[1] == 0


def test_the_intensity_image_is_the_weighted_sum():
    rgb = np.zeros((2, 3, 3), F32)
    rgb[0, 0], rgb[0, 1], rgb[0, 2], rgb[1, 0], rgb[1, 1] = (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (10, 20, 30)
    y = ref.intensity(rgb)
    assert y.dtype == F32 and y.shape == (2, 3) and y[1, 2] == 0.0
    assert y[0, 0] == (F32(0.299) * F32(255) + F32(0.587) * F32(255) + F32(0.114) * F32(255)) / F32(255)
    assert abs(float(y[0, 0]) - 1.0) < 1e-6 and abs(float(y[0, 1]) - 0.299) < 1e-7 and abs(float(y[1, 0]) - 0.114) < 1e-7
    assert y[1, 1] == ((F32(0.299) * F32(10) + F32(0.587) * F32(20)) + F32(0.114) * F32(30)) / F32(255)
    assert np.isnan(ref.intensity(np.full((1, 1, 3), np.nan, F32))).all()


# ---- (b) the wall ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def walls():
    return {slant: ref.wall_case(slant) for slant in (0.0, 0.3)}


def _information(out, extra=None):
    return information_from_sums(out, mapping.INFO_MIN_EIG, extra)


@pytest.mark.parametrize("slant", [0.0, 0.3])
def test_depth_leaves_the_wall_open_and_colour_closes_it(slant, walls, capsys):
    c = walls[slant]
    start = np.eye(4, dtype=F32)
    geo = info.pose_info(c["means"], start, c["intr"], c["depth"], KEEP, BEYOND, KAPPA, NEAR)
    gi = _information(geo)
    assert gi.used > 18000 and gi.weak() and int((gi.eigenvalues < mapping.INFO_MIN_EIG).sum()) == 3
    if slant == 0.0:
        assert not gi.eigenvalues[:3].any()  # n = (0, 0, 1) exactly: exact zeros
    out, extra = ref.pose_info(c["means"], c["colors"], start, c["intr"], c["depth"], c["image"], KEEP, BEYOND, KAPPA,
                               NEAR, SCALE, RMAX)
    pi = _information(out, extra)
    assert not pi.weak() and pi.eigenvalues[0] > 5 * mapping.INFO_MIN_EIG
    assert (pi.used, pi.tested) == (gi.used, gi.tested) and pi.photo_used == pi.used  # every used row, on this wall
    assert 0.0 < pi.photo_rss <= pi.rss and pi.covariance() is not None and pi.step() is not None
    # the alignment: depth alone does not move in the plane, colour converges onto the floor of the linear model
    e0 = ref.pose_error(start, c["truth"])
    P, _, taken, _, hist, _, _ = align.pose_align(c["means"], start, c["intr"], c["depth"], KEEP, BEYOND, KAPPA, NEAR,
                                                  *ALIGN)
    eg = ref.pose_error(P, c["truth"])
    P, work, taken, done, hist, xis, sums = ref.pose_align(c["means"], c["colors"], start, c["intr"], c["depth"],
                                                           c["image"], KEEP, BEYOND, KAPPA, NEAR, SCALE, RMAX, *ALIGN)
    ep = ref.pose_error(P, c["truth"])
    with capsys.disabled():
        print(f"[photo] wall slant {slant}: used {pi.used} photo {pi.photo_used}; eigenvalues of H / used, depth "
              f"{gi.eigenvalues[:3]}, with colour {pi.eigenvalues[:3]}; start {e0[0]:.3e} m {e0[1]:.3e} deg; depth "
              f"alone {eg[0]:.3e} m {eg[1]:.3e} deg; with colour {align.NAMES[hist[-1, 0]]} after {taken} steps "
              f"{ep[0]:.3e} m {ep[1]:.3e} deg")
    assert abs(e0[0] - 0.0144) < 1e-4 and abs(e0[1] - 0.3) < 1e-3
    if slant == 0.0:
        assert eg == e0  # every step is exactly 0
    else:
        assert eg[0] > 0.8 * e0[0] and eg[1] > 0.8 * e0[1]  # what the slant sees of x is a fifth of the move
    assert hist[-1, 0] == align.CONVERGED and done == 1 and taken < 8
    assert ep[0] <= WALL_BOUND[slant][0] and ep[1] <= WALL_BOUND[slant][1], ep


def test_a_smaller_scale_is_slower_and_a_tiny_one_stays_weak(walls):
    """What the documented default rests on: 0.05 leaves the smallest eigenvalue below INFO_MIN_EIG, 0.1 converges later
    than 0.2."""
    c = walls[0.0]
    start = np.eye(4, dtype=F32)
    eig, steps = {}, {}
    for s in (0.05, 0.1, 0.2):
        out, extra = ref.pose_info(c["means"], c["colors"], start, c["intr"], c["depth"], c["image"], KEEP, BEYOND, KAPPA,
                                   NEAR, s, RMAX)
        eig[s] = float(_information(out, extra).eigenvalues[0])
    assert eig[0.05] < mapping.INFO_MIN_EIG < eig[0.1] < eig[0.2]
    assert 3.5 < eig[0.2] / eig[0.1] < 4.5  # the colour share of H goes with the square of the scale
    for s in (0.1, 0.2):
        _, _, taken, _, hist, _, _ = ref.pose_align(c["means"], c["colors"], start, c["intr"], c["depth"], c["image"],
                                                    KEEP, BEYOND, KAPPA, NEAR, s, RMAX, *ALIGN)
        assert hist[-1, 0] == align.CONVERGED
        steps[s] = taken
    assert steps[0.2] < steps[0.1]


# ---- (c) g is the gradient of the summed cost ----------------------------------------------------------------------
def test_g_is_the_gradient_of_half_the_squared_residuals(walls):
    """At the start pose on the slanted wall (both kinds of residual are there) the camera is turned and moved by +-h
    along each of the six axes, w2c' = exp(h e_k^) w2c.  h = 1e-3 moves a row by 0.1 pixel at the most, the rows project
    onto pixel centres, so no row changes its pixel and the used sets are asserted to be the same: the cost
    1/2 sum (r^2 + (s rc)^2) is then smooth, and its central difference misses g_k by the third-order term of the
    rotation, h^2 relative, and by the float32 rounding of the residuals (1e-7 relative per row, summed with random
    signs): 1e-3 of the largest |g_k| bounds both with two orders to spare."""
    c = walls[0.3]
    args = (c["intr"], c["depth"], c["image"], KEEP, BEYOND, KAPPA, NEAR, SCALE, RMAX)
    start = np.eye(4)

    def at(w2c):
        tested, used, J, photo, Jc = ref.rows(c["means"], c["colors"], w2c.astype(F32), *args)
        cost = 0.5 * (np.sum(J[used, 6].astype(np.float64) ** 2) + np.sum(Jc[photo, 6].astype(np.float64) ** 2))
        return cost, used, photo

    _, used0, photo0 = at(start)
    out, extra = ref.pose_info(c["means"], c["colors"], start.astype(F32), *args)
    g = ref.unpack(out)[1]
    assert used0.sum() > 18000 and photo0.sum() == used0.sum() and np.abs(g[:3]).max() > 1.0 and np.abs(g[3:]).max() > 1.0
    h, fd = 1e-3, np.zeros(6)
    for k in range(6):
        e = np.zeros(6)
        e[k] = h
        up, used_up, photo_up = at(ref.twist_pose(e) @ start)
        down, used_down, photo_down = at(ref.twist_pose(-e) @ start)
        for flags, want in ((used_up, used0), (used_down, used0), (photo_up, photo0), (photo_down, photo0)):
            assert np.array_equal(flags, want), k
        fd[k] = (up - down) / (2 * h)
    assert np.abs(fd - g).max() <= 1e-3 * np.abs(g).max(), (fd, g)


# ---- (d) the entry points: prototypes and refusals -----------------------------------------------------------------
BAD_ARG = -1
GOOD = dict(n_rows=1000, n_poses=2, fx=50.0, fy=40.0, cx=31.5, cy=23.5, width=64, height=48, keep=0.95, beyond=1.05,
            kappa=1e-3, near_plane=0.01, max_steps=4, damping=1e-3, min_used=7, max_rot=0.2, max_trans=0.3, eps_rot=1e-6,
            eps_trans=1e-6, photo_scale=0.2, photo_max_residual=0.1)
GOOD_INTR = (50.0, 40.0, 31.5, 23.5)
GOOD_MAX_ROWS = ref.max_rows(GOOD_INTR, 64, 48, 0.95, 0.2, 0.1)
GEOMETRIC = dict(gsl_map_pose_info_photo="gsl_map_pose_info", gsl_map_pose_align_photo="gsl_map_pose_align",
                 gsl_map_pose_align_batch_photo="gsl_map_pose_align_batch")
PHOTO_REFUSED = [
    ("NULL colors", dict(colors=None)), ("NULL intensity", dict(intensity=None)),
    ("photo_scale < 0", dict(photo_scale=-1e-3)), ("photo_scale > 16", dict(photo_scale=16.000002)),
    ("NaN photo_scale", dict(photo_scale=float("nan"))), ("inf photo_scale", dict(photo_scale=float("inf"))),
    ("photo_max_residual < 0", dict(photo_max_residual=-1e-3)), ("photo_max_residual > 1", dict(photo_max_residual=1.0000001)),
    ("NaN photo_max_residual", dict(photo_max_residual=float("nan"))),
    ("a sum could overflow", dict(n_rows=GOOD_MAX_ROWS + 1)),
    ("the geometric bound would still take it", dict(n_rows=info.max_rows(GOOD_INTR, 64, 48, 0.95))),
    # ... and what the geometric twin refuses
    ("NULL means", dict(means=None)), ("NULL w2c", dict(w2c=None)), ("NULL depth", dict(depth=None)),
    ("n_rows == 0", dict(n_rows=0)), ("n_rows < 0", dict(n_rows=-5)), ("n_rows == 2^31", dict(n_rows=1 << 31)),
    ("a NaN principal point", dict(cy=float("nan"))), ("width <= 0", dict(width=0)), ("height <= 0", dict(height=-3)),
    ("2^31 pixels", dict(width=65536, height=32768)), ("fx == 0", dict(fx=0.0)), ("fy == 0", dict(fy=0.0)),
    ("keep == 0", dict(keep=0.0)), ("keep > 1", dict(keep=1.0000001)), ("NaN keep", dict(keep=float("nan"))),
    ("beyond < 1", dict(beyond=0.9999999)), ("inf beyond", dict(beyond=float("inf"))),
    ("kappa < 0", dict(kappa=-1e-3)), ("NaN kappa", dict(kappa=float("nan"))),
]
OWN_REFUSED = {
    "gsl_map_pose_info_photo": [("NULL out", dict(out=None)), ("NULL extra", dict(extra=None))],
    "gsl_map_pose_align_photo": [
        ("NULL sums", dict(sums=None)), ("NULL work", dict(work=None)), ("NULL state", dict(state=None)),
        ("NULL history", dict(history=None)), ("max_steps == 0", dict(max_steps=0)), ("max_steps == 33", dict(max_steps=33)),
        ("min_used == 6", dict(min_used=6)), ("damping < 0", dict(damping=-1.0)), ("max_rot == 0", dict(max_rot=0.0)),
        ("NaN max_trans", dict(max_trans=float("nan"))), ("eps_rot < 0", dict(eps_rot=-1.0)),
        ("inf eps_trans", dict(eps_trans=float("inf")))],
}
OWN_REFUSED["gsl_map_pose_align_batch_photo"] = OWN_REFUSED["gsl_map_pose_align_photo"] + [
    ("n_poses == 0", dict(n_poses=0)), ("n_poses == 17", dict(n_poses=17))]
INTENSITY_REFUSED = [("NULL rgb", dict(rgb=None)), ("NULL intensity", dict(intensity=None)), ("width <= 0", dict(width=0)),
                     ("height <= 0", dict(height=-1)), ("2^31 pixels", dict(width=65536, height=32768))]


def refusals():
    """[(function, what, the named arguments over GOOD)] of every refusal of the five entry points."""
    out = [("gsl_map_photo_intensity", what, dict(dict(width=64, height=48), **over)) for what, over in INTENSITY_REFUSED]
    for fn in GEOMETRIC:
        out += [(fn, what, dict(GOOD, **over)) for what, over in PHOTO_REFUSED + OWN_REFUSED[fn]]
    return out


def call_with(lib, fn, params, named, pointers):
    args = []
    for c_type, name in params:
        if name == "stream":
            args.append(None)
        elif name in named:
            args.append(named[name])
        else:
            assert "*" in c_type, (fn, name)
            args.append(pointers[name])
    return getattr(lib, fn)(*args)


def test_the_prototypes_follow_their_twins(repo_root):
    protos = prototypes(repo_root)
    tail = [("const float*", "colors"), ("const float*", "intensity"), ("float", "photo_scale"),
            ("float", "photo_max_residual")]
    for fn, twin in GEOMETRIC.items():
        ret, params = protos[fn]
        want = protos[twin][1][:-1] + tail + ([("int64_t*", "extra")] if fn == "gsl_map_pose_info_photo" else []) + [
            ("void*", "stream")]
        assert ret == "int" and params == want, fn
        assert len(_lib._SIGNATURES[fn][1]) == len(params)
    assert protos["gsl_map_photo_intensity"] == ("int", [("const float*", "rgb"), ("int", "width"), ("int", "height"),
                                                         ("float*", "intensity"), ("void*", "stream")])
    assert [n for _, n in protos["gsl_map_info_photo_max_rows"][1]] == [
        "fx", "fy", "cx", "cy", "width", "height", "keep", "photo_scale", "photo_max_residual"]
    csrc = os.path.join(repo_root, "gsplatloc_amd", "csrc")
    where = dict(gsl_map_photo_intensity="map_photo.hip", gsl_map_info_photo_max_rows="map_photo.hip",
                 gsl_map_pose_info_photo="map_photo.hip", gsl_map_pose_align_photo="map_align.hip",
                 gsl_map_pose_align_batch_photo="map_align_batch.hip")
    for fn, name in where.items():
        src = open(os.path.join(csrc, name)).read()
        m = re.search(r'extern "C" \w+ ' + fn + r"\((.*?)\)\s*\{", src, flags=re.S)
        assert m, fn
        defined = [re.fullmatch(r"\s*(.*?)\s*(\w+)\s*", p, flags=re.S).groups() for p in m.group(1).split(",")]
        assert [(" ".join(t.split()), n) for t, n in defined] == protos[fn][1], fn
    assert "map_photo.hip" in open(os.path.join(csrc, "Makefile")).read()
    src = open(os.path.join(csrc, "map_photo.hip")).read() + open(os.path.join(csrc, "map_info_dev.h")).read()
    assert "#pragma clang fp contract(off)" in src and "atomicAdd(float" not in src and "hipMemset" not in src
    # the one copy: nobody but map_info_dev.h writes the rule out
    for name in ("map_photo.hip", "map_info.hip", "map_align.hip", "map_align_batch.hip"):
        assert "info_fix(" not in open(os.path.join(csrc, name)).read().split("#include", 1)[1], name
    # the constants of the kernel are the mirror's and the host's
    dev = open(os.path.join(csrc, "map_info_dev.h")).read()
    for name, value in (("INFO_PHOTO_MAX_A", ref.PHOTO_MAX_A), ("INFO_PHOTO_MAX_DEPTH", ref.PHOTO_MAX_DEPTH),
                        ("INFO_PHOTO_MAX_SCALE", ref.PHOTO_MAX_SCALE)):
        assert float(re.search(r"constexpr float " + name + r" = ([\d.]+)f;", dev).group(1)) == float(value), name
    assert mapping.INFO_PHOTO_MAX_SCALE == ref.PHOTO_MAX_SCALE


def test_entry_points_reject_bad_arguments_before_any_launch(repo_root):
    """Every row is refused on the host: the pointers are one dummy HOST buffer, a launch (the zeroing of out is one)
    would give GSL_ERR_HIP or worse."""
    lib, protos = _lib.load_library(), prototypes(repo_root)
    buf = ctypes.create_string_buffer(b"\x7f" * 1024, 1024)
    seen = set()
    for fn, what, named in refusals():
        params = protos[fn][1]
        pointers = {n: ctypes.addressof(buf) for t, n in params if "*" in t}
        assert set(named) >= {n for t, n in params if "*" not in t}, (fn, what)
        assert call_with(lib, fn, params, named, pointers) == BAD_ARG, (fn, what)
        seen.add(fn)
    assert len(seen) == 4 and buf.raw == b"\x7f" * 1024  # nothing wrote to the buffer


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_the_photo_kernels_stay_in_registers():
    """The photo instantiations of info_sum_rows: no scratch, no accumulation registers, the table of 32 sums in LDS, at
    least four waves per SIMD (the grid cap is four workgroups per CU); the intensity kernel needs next to nothing."""
    res = _resources("map_photo.hip")
    hit = [v for k, v in res.items() if "k_map_pose_info_photo" in k]
    hit += [v for k, v in _resources("map_align_batch.hip").items() if "k_map_batch_photo_info" in k]
    assert len(hit) == 2
    for r in hit:
        assert r["ScratchSize"] == 0 and r["AGPRs"] == 0 and r["LDS"] == 32 * 8 and r["VGPRs"] <= 128, r
        assert r["Occupancy"] >= 4, r
    small = [v for k, v in res.items() if "k_map_photo_intensity" in k]
    assert len(small) == 1 and small[0]["ScratchSize"] == 0 and small[0]["LDS"] == 0 and small[0]["Occupancy"] == 8


# ---- (e) the row bound ----------------------------------------------------------------------------------------------
def test_the_row_bound():
    lib = _lib.load_library()
    K = replica_intrinsics(640, 480)
    intr = base.intrinsics(K)
    # the condition: a map of four frames of the Replica camera at 640 x 480, at the largest scale and residual
    assert lib.gsl_map_info_photo_max_rows(*intr, 640, 480, 0.95, 16.0, 1.0) >= 4 * 640 * 480
    assert ref.max_rows(intr, 640, 480, 0.95, 16.0, 1.0) >= 4 * 640 * 480
    cases = [(GOOD_INTR, 64, 48, 0.95, 0.2, 0.1), (intr, 640, 480, 0.95, 16.0, 1.0), (intr, 640, 480, 0.95, 0.0, 0.0),
             ((80.0, 80.0, 79.5, 59.5), 160, 120, 0.95, 0.2, 0.1), ((1.0, 1.0, 100.0, 100.0), 200, 200, 0.01, 1.0, 1.0),
             ((1e-3, 1e-3, 0.0, 0.0), 3, 3, 1.0, 16.0, 0.5), ((-50.0, 40.0, 31.5, 23.5), 64, 48, 1.0, 0.2, 0.1)]
    for i, w, h, keep, s, r in cases:
        got, want = lib.gsl_map_info_photo_max_rows(*i, w, h, keep, s, r), ref.max_rows(i, w, h, keep, s, r)
        assert abs(got - want) <= max(1, want >> 40) and 0 < got <= 2 ** 31 - 1, (i, got, want)
        assert got <= lib.gsl_map_info_max_rows(*i, w, h, keep)  # never above the geometric bound
    # B and Bc bound every entry of J and Jc: with them no sum of n rows, two terms each, leaves 63 bits
    i, w, h, keep, s, r = cases[1]
    tx, ty = (w - 1.5 - i[2]) / i[0], (h - 1.5 - i[3]) / i[1]
    S = math.sqrt(1.0 + tx * tx + ty * ty)
    B, Bc = 64.0 * S * (1.0 + 1.0 / keep), max(16.0 * S * 8.0 * math.sqrt(3.0), s * r)
    assert ref.max_rows(i, w, h, keep, s, r) * ((B * B + Bc * Bc) * 2.0 ** 20 + 2.0) < 2.0 ** 63
    # ... and the bound on Jc holds on rows at the gates: |a| at 8, z just below 16, at the image's corner
    z, a = float(np.nextafter(F32(16.0), F32(0))), 8.0
    p = np.array([tx * z, ty * z, z])
    assert np.abs(np.cross(p, [a, -a, a])).max() <= Bc and np.abs(np.cross(p, [a, a, -a])).max() <= Bc
    for bad in ((0.0, 40.0, 31.5, 23.5, 64, 48, 0.95, 0.2, 0.1), (50.0, 40.0, 31.5, 23.5, 0, 48, 0.95, 0.2, 0.1),
                (50.0, 40.0, 31.5, 23.5, 64, 48, 0.0, 0.2, 0.1), (50.0, 40.0, float("nan"), 23.5, 64, 48, 0.95, 0.2, 0.1),
                (50.0, 40.0, 31.5, 23.5, 64, 48, 0.95, -0.1, 0.1), (50.0, 40.0, 31.5, 23.5, 64, 48, 0.95, 16.5, 0.1),
                (50.0, 40.0, 31.5, 23.5, 64, 48, 0.95, float("nan"), 0.1), (50.0, 40.0, 31.5, 23.5, 64, 48, 0.95, 0.2, 1.5),
                (50.0, 40.0, 31.5, 23.5, 64, 48, 0.95, 0.2, -0.1), (50.0, 40.0, 31.5, 23.5, 64, 48, 0.95, 0.2, float("nan"))):
        assert lib.gsl_map_info_photo_max_rows(*bad) == 0, bad


# ---- (f) MapConfig, PoseInformation, the host layer's checks --------------------------------------------------------
def test_map_config_validation():
    c = MapConfig()
    assert (c.photo_scale, c.photo_max_residual) == (None, 0.1)
    for on in (dict(info=True), dict(align=True), dict(loop=True, origins=True)):
        assert MapConfig(photo_scale=0.2, **on).photo_scale == 0.2
    assert MapConfig(info=True, photo_scale=0, photo_max_residual=0).photo_scale == 0
    assert MapConfig(info=True, photo_scale=16.0, photo_max_residual=1.0).photo_max_residual == 1.0
    assert MapConfig(photo_max_residual=0.5).photo_max_residual == 0.5  # without a scale it is only a number
    with pytest.raises(ValueError, match="photo_scale needs info=True, align=True or loop=True"):
        MapConfig(photo_scale=0.2)
    with pytest.raises(ValueError, match="photo_scale needs"):
        MapConfig(photo_scale=0.2, reloc=True, origins=True, refine=True)
    bad = dict(photo_scale=[-0.1, 16.5, float("nan"), float("inf"), True, "0.2"],
               photo_max_residual=[-0.1, 1.5, float("nan"), True, None, "0.1"])
    for field, values in bad.items():
        for v in values:
            with pytest.raises(ValueError, match=field):
                MapConfig(info=True, **{field: v})


def test_pose_information_carries_the_photometric_share():
    out = np.zeros(30, np.int64)
    out[27], out[28], out[29] = 3 << 20, 10, 12
    plain = information_from_sums(out)
    assert (plain.photo_used, plain.photo_rss, plain.rss) == (0, 0.0, 3.0)
    with_colour = information_from_sums(out, 0.5, np.array([9, 1 << 19], np.int64))
    assert (with_colour.photo_used, with_colour.photo_rss, with_colour.rss, with_colour.min_eig) == (9, 0.5, 3.0, 0.5)
    assert PoseInformation(np.eye(6), np.zeros(6), 1.0, 10, 12).photo_used == 0  # the fields of before, in their order
    assert "overstated" in PoseInformation.covariance.__doc__


def test_the_host_layer_checks_its_photometric_arguments():
    w, h = base.PW, base.PH
    depth, means = base.plane_case()
    m = GaussianMap(w, h, MapConfig(info=True, photo_scale=0.25, photo_max_residual=0.5), "cpu")
    image = torch.rand(h, w)
    got = m._photo_params(image, None, None)
    assert torch.equal(got[0], image) and got[1:] == (0.25, 0.5)
    assert m._photo_params(image, 0.1, 0.2)[1:] == (float(F32(0.1)), float(F32(0.2)))
    assert m._photo_params(None, None, None) is None
    for bad, match in ((dict(photo_scale=-1.0), "photo_scale"), (dict(photo_scale=17.0), "photo_scale"),
                       (dict(photo_max_residual=1.5), "photo_max_residual"),
                       (dict(photo_max_residual=float("nan")), "photo_max_residual")):
        with pytest.raises(ValueError, match=match):
            m.pose_information(depth, base.PK, torch.eye(4), NEAR, intensity=image, **bad)
    with pytest.raises(ValueError, match="intensity"):
        m.pose_information(depth, base.PK, torch.eye(4), NEAR, intensity=torch.rand(h, w + 1))
    with pytest.raises(ValueError, match="need intensity"):
        m.align_pose(depth, base.PK, torch.eye(4), NEAR, photo_scale=0.2)
    with pytest.raises(ValueError, match="need intensity"):
        m.align_poses(depth, base.PK, [torch.eye(4)], NEAR, photo_max_residual=0.2)
    plain = GaussianMap(w, h, MapConfig(info=True), "cpu")
    with pytest.raises(ValueError, match="photo_scale"):
        plain.pose_information(depth, base.PK, torch.eye(4), NEAR, intensity=image)  # nobody names a scale
    # an empty map answers without a launch, with or without an image
    empty = m.pose_information(depth, base.PK, torch.eye(4), NEAR, intensity=image)
    assert (empty.used, empty.photo_used, empty.weak()) == (0, 0, True)
    assert m.align_pose(depth, base.PK, torch.eye(4), NEAR, intensity=image).status == "FEW"
    with pytest.raises(ValueError, match="rgb"):
        m.intensity(torch.zeros(h, w))
    m.n_live = 3
    for call in (lambda: m.intensity(torch.zeros(h, w, 3)),
                 lambda: m.pose_information(depth, base.PK, torch.eye(4), NEAR, intensity=image),
                 lambda: m.align_pose(depth, base.PK, torch.eye(4), NEAR, intensity=image),
                 lambda: m.align_poses(depth, base.PK, [torch.eye(4)], NEAR, intensity=image)):
        with pytest.raises(AssertionError, match="no CPU path"):
            call()


def test_the_options_of_the_evaluation_driver(tmp_path, capsys):
    from gsplatloc_amd import eval as ev

    with pytest.raises(ValueError, match="map_photo_scale belongs to the map mode"):
        ev.evaluate_room(None, 200, 3, sequential=True, map_photo_scale=0.2)
    with pytest.raises(ValueError, match="map_info, map_align or map_loop"):
        ev.evaluate_room(None, 200, 3, sequential=True, map_mode=True, map_photo_scale=0.2)
    with pytest.raises(ValueError, match="map_photo_max_residual"):
        ev.evaluate_room(None, 200, 3, sequential=True, map_mode=True, map_info=True, map_photo_max_residual=0.2)
    for extra, word in ((["--sequential", "--map", "--map-photo-scale", "0.2"], "needs --map-info"),
                        (["--sequential", "--map", "--map-info", "--map-photo-max-residual", "0.2"],
                         "needs --map-photo-scale")):
        with pytest.raises(SystemExit):
            ev.main(["--root", str(tmp_path)] + extra)
        assert word in capsys.readouterr().err
