"""Exposure compensation for the photometric term (csrc/map_exposure.hip, MapConfig.photo_exposure), the parts that
need no GPU: the numpy mirror tests/map_exposure_ref.py on rows it can be checked on by hand; each status where it is
expected; the entry points against their prototypes and every refusal, with host pointers; the kernels' resources;
MapConfig and the host layer's own checks; and the experiment the feature rests on.

The wall (tests/map_photo_ref.wall_case(): 160x120, the textured plane z = 2 m, the map is frame 0 back-projected, the
query 0.3 degrees and 14.4 mm away, aligned from the identity start with photo_scale 0.2, photo_max_residual 0.1, 8
steps) with a query image of 0.85 rgb + 255 * 0.06.  A float64 prototype of the estimator measured a gain 7.5e-4 and an
offset 4.1e-4 from the exact inverse (1 / 0.85, -0.06 / 0.85), and an alignment on the corrected image 1.18 times as far
from the truth as the same-exposure alignment and 0.016 times as far as the uncorrected one.  The float32 / fixed-point
mirror of this file measures: gain 1.1755924 (8.8e-4 off), offset -0.07021219 (3.8e-4 off), 19200 rows used in both
passes; translation error 1.696e-5 m as rendered, 1.273e-3 m uncorrected, 2.064e-5 m corrected: 1.217 x and 0.0162 x.
The bounds asserted are the issue's: 2e-3, 1e-3, 2 x and 0.1 x."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from gsplatloc_amd import _lib, mapping
from gsplatloc_amd.mapping import Exposure, GaussianMap, MapConfig
from tests import map_exposure_ref as ref
from tests import map_photo_ref as photo
from tests.test_abi import prototypes
from tests.test_kernel_resources import HIPCC, _resources
from tests.test_map_photo_cpu import call_with

F32 = np.float32
NEAR = 0.01
KEEP, BEYOND, KAPPA = photo.keep_of(0.05), photo.beyond_of(0.05), F32(1e-3)
ALIGN = (8, 1e-3, 7, math.radians(12.8), 0.32, math.radians(1.5e-4), 3e-5)  # MapConfig's defaults
EYE = np.eye(4, dtype=F32)
# rows on pixel centres: fx = fy = 8, cx = 24, cy = 8 on a 48x17 image of depth 2 m (tests/test_gpu_map_photo.py)
SW, SH = 48, 17
SINTR = (8.0, 8.0, 24.0, 8.0)


def centre_rows():
    """(means, depth): one row on the centre of every pixel of the 48x17 image, 2 m away (dyadic: exact)."""
    depth = np.full((SH, SW), 2.0, F32)
    means = np.array([[(u - SINTR[2]) / 8.0 * 2.0, (v - SINTR[3]) / 8.0 * 2.0, 2.0] for v in range(SH)
                      for u in range(SW)], F32)
    return means, depth


def grey_rows(seed=3, lo=0.1, hi=0.9):
    """(colors [n,3], Yi [H,W] float32): a grey per pixel, uniform in lo .. hi, and its intensity as the rule makes it."""
    g = np.random.default_rng(seed).uniform(lo, hi, SW * SH).astype(F32)
    colors = np.repeat(g[:, None], 3, axis=1)
    yi = (ref.WR * g + ref.WG * g) + ref.WB * g
    return colors, yi.reshape(SH, SW)


def _estimate(means, colors, depth, image, **over):
    p = dict(zip(("sat_lo", "sat_hi", "max_residual", "passes", "min_used", "gain_min", "gain_max", "offset_max",
                  "min_var"), ref.DEFAULTS))
    p.update(over)
    return ref.estimate(means, colors, EYE, SINTR, depth, image, KEEP, BEYOND, NEAR, *p.values())


# ---- (a) the mirror -------------------------------------------------------------------------------------------------
def test_rows_on_pixel_centres_give_the_gain_and_the_offset():
    means, depth = centre_rows()
    colors, yi = grey_rows()
    image = (F32(0.5) * yi + F32(0.125)).astype(F32)
    out, params, record = _estimate(means, colors, depth, image, gain_max=4.0, offset_max=0.5)
    assert out[5] == out[6] == SW * SH  # every row is seen and used, border pixels included
    assert [r[0] for r in record] == [ref.OK, ref.OK]
    assert abs(float(params[0]) - 2.0) <= 1e-6 and abs(float(params[1]) + 0.25) <= 1e-6, params
    assert params[2] == params[1] * F32(255.0) and params[3] == 0.0
    assert abs(record[-1][3] - 2.0) <= 1e-6 and abs(record[-1][4] + 0.25) <= 1e-6
    assert abs(record[-1][5]) <= SW * SH * 2.0 ** -19  # the residual is the fixed point's rounding
    # the sums are what they say
    x, y = image.reshape(-1), yi.reshape(-1)
    assert out[1] == int(np.rint(x * F32(2 ** 20)).astype(np.int64).sum())
    assert out[2] == int(np.rint((x * y) * F32(2 ** 20)).astype(np.int64).sum())
    # ... and the correction is the inverse: the corrected image has the rows' intensities
    rgb = np.repeat((image * F32(255.0))[..., None], 3, axis=-1)
    fixed = photo.intensity(ref.apply(rgb, params))
    assert np.abs(fixed - yi).max() <= 2e-6


def test_apply_clips_and_keeps_a_nan():
    rgb = np.array([[[0.0, 255.0, 100.0], [np.nan, np.inf, -np.inf], [-5.0, 300.0, 127.5]]], F32)
    got = ref.apply(rgb, ref.params_of(2.0, -0.25))
    want = np.array([[[0.0, 255.0, 136.25], [np.nan, 255.0, 0.0], [0.0, 255.0, 191.25]]], F32)
    assert np.array_equal(got, want, equal_nan=True) and got.dtype == F32
    assert np.array_equal(ref.apply(rgb, ref.IDENTITY), np.clip(rgb, 0, 255), equal_nan=True)


def test_each_status_arises_where_expected_and_leaves_the_parameters_alone():
    means, depth = centre_rows()
    colors, yi = grey_rows()
    image = (F32(0.5) * yi + F32(0.125)).astype(F32)
    n = SW * SH
    # FEW: one row short
    out, params, record = _estimate(means, colors, depth, image, min_used=n + 1, gain_max=4.0, offset_max=0.5)
    assert [r[0] for r in record] == [ref.FEW, ref.FEW] and np.array_equal(params, ref.IDENTITY)
    assert record[0][1:5] == (n, n, 1.0, 0.0) and record[0][5] == 0.0
    assert _estimate(means, colors, depth, image, min_used=n, gain_max=4.0, offset_max=0.5)[2][0][0] == ref.OK
    # FLAT: a constant image
    out, params, record = _estimate(means, colors, depth, np.full((SH, SW), 0.5, F32))
    assert [r[0] for r in record] == [ref.FLAT, ref.FLAT] and np.array_equal(params, ref.IDENTITY)
    assert record[0][1] == n and out[5] == record[1][1] < n  # the ended pass still counts, behind the gate at (1, 0)
    # RANGE: the gain is 2 and a step beyond what is allowed; the offset alone
    out, params, record = _estimate(means, colors, depth, image, gain_max=1.999, offset_max=0.5)
    assert [r[0] for r in record] == [ref.RANGE, ref.RANGE] and np.array_equal(params, ref.IDENTITY)
    assert abs(record[0][3] - 2.0) <= 1e-6 and record[1][3:] == (1.0, 0.0, 0.0)  # solved and recorded; then ended
    out, params, record = _estimate(means, colors, depth, image, gain_max=4.0, offset_max=0.2)
    assert record[0][0] == ref.RANGE and np.array_equal(params, ref.IDENTITY)
    # a second pass that fails leaves what the first one solved: the gate is 0 and no row passes it exactly
    out, params, record = _estimate(means, colors, depth, (F32(0.51) * yi + F32(0.125)).astype(F32), gain_max=4.0,
                                    offset_max=0.5, max_residual=0.0, min_used=n // 2)
    assert [r[0] for r in record] == [ref.OK, ref.FEW] and out[5] < n // 2 and out[6] == n
    assert params[0] == F32(record[0][3]) and params[1] == F32(record[0][4]) and record[1][3] == float(params[0])
    # clipped pixels do not vote: the saturation range applies to the image and to the row
    dark = image.copy()
    dark[0, :] = 0.01
    assert _estimate(means, colors, depth, dark, gain_max=4.0, offset_max=0.5)[0][5] == n - SW
    black = colors.copy()
    black[:7] = 0.0
    assert _estimate(means, black, depth, image, gain_max=4.0, offset_max=0.5)[0][5] == n - 7


# ---- (b) the wall ---------------------------------------------------------------------------------------------------
def test_the_wall_under_another_exposure(capsys):
    c = photo.wall_case()
    raw = (F32(0.85) * c["rgb"] + F32(255.0 * 0.06)).astype(F32)
    image = photo.intensity(raw)
    assert 0.1 < image.min() and image.max() < 0.9  # no residual reaches the gate, nothing clips
    out, params, record = ref.estimate(c["means"], c["colors"], EYE, c["intr"], c["depth"], image, KEEP, BEYOND, NEAR,
                                       *ref.DEFAULTS)
    assert [r[0] for r in record] == [ref.OK, ref.OK] and out[5] > 18000
    gain_err, offset_err = abs(float(params[0]) - 1.0 / 0.85), abs(float(params[1]) + 0.06 / 0.85)
    corrected = photo.intensity(ref.apply(raw, params))

    def align_on(img):
        P = photo.pose_align(c["means"], c["colors"], EYE, c["intr"], c["depth"], img, KEEP, BEYOND, KAPPA, NEAR, 0.2, 0.1,
                             *ALIGN)[0]
        return photo.pose_error(P, c["truth"])

    same, off, fixed = align_on(c["image"]), align_on(image), align_on(corrected)
    with capsys.disabled():
        print(f"[exposure] wall: gain {float(params[0]):.7f} ({gain_err:.2e} off) offset {float(params[1]):.7f} "
              f"({offset_err:.2e} off) used {out[5]}; as rendered {same[0]:.3e} m {same[1]:.3e} deg; uncorrected "
              f"{off[0]:.3e} m {off[1]:.3e} deg; corrected {fixed[0]:.3e} m {fixed[1]:.3e} deg: "
              f"{fixed[0] / same[0]:.3f} x, {fixed[0] / off[0]:.4f} x")
    assert gain_err <= 2e-3 and offset_err <= 1e-3
    assert fixed[0] <= 2.0 * same[0] and fixed[0] <= 0.1 * off[0]


# ---- (c) the entry points: prototypes and refusals -----------------------------------------------------------------
BAD_ARG = -1
GOOD = dict(n_rows=1000, fx=50.0, fy=40.0, cx=31.5, cy=23.5, width=64, height=48, keep=0.95, beyond=1.05,
            near_plane=0.01, sat_lo=0.02, sat_hi=0.98, max_residual=0.1, passes=2, min_used=256, gain_min=0.5,
            gain_max=2.0, offset_max=0.25, min_var=1e-4)
NAN, INF = float("nan"), float("inf")
ESTIMATE_REFUSED = [
    ("NULL means", dict(means=None)), ("NULL colors", dict(colors=None)), ("NULL w2c", dict(w2c=None)),
    ("NULL depth", dict(depth=None)), ("NULL intensity", dict(intensity=None)), ("NULL sums", dict(sums=None)),
    ("NULL params", dict(params=None)), ("NULL record", dict(record=None)),
    ("n_rows == 0", dict(n_rows=0)), ("n_rows < 0", dict(n_rows=-5)), ("n_rows == 2^31", dict(n_rows=1 << 31)),
    ("width <= 0", dict(width=0)), ("height <= 0", dict(height=-3)), ("2^31 pixels", dict(width=65536, height=32768)),
    ("fx == 0", dict(fx=0.0)), ("fy == 0", dict(fy=0.0)),
    ("keep == 0", dict(keep=0.0)), ("keep > 1", dict(keep=1.0000001)), ("NaN keep", dict(keep=NAN)),
    ("beyond < 1", dict(beyond=0.9999999)), ("inf beyond", dict(beyond=INF)), ("NaN beyond", dict(beyond=NAN)),
    ("sat_lo < 0", dict(sat_lo=-1e-3)), ("sat_lo == sat_hi", dict(sat_lo=0.5, sat_hi=0.5)),
    ("sat_lo > sat_hi", dict(sat_lo=0.6, sat_hi=0.5)), ("sat_hi > 1", dict(sat_hi=1.0000001)),
    ("NaN sat_lo", dict(sat_lo=NAN)), ("NaN sat_hi", dict(sat_hi=NAN)),
    ("max_residual < 0", dict(max_residual=-1e-3)), ("inf max_residual", dict(max_residual=INF)),
    ("NaN max_residual", dict(max_residual=NAN)),
    ("passes == 0", dict(passes=0)), ("passes == 5", dict(passes=5)), ("min_used == 0", dict(min_used=0)),
    ("gain_min == 0", dict(gain_min=0.0)), ("gain_min > 1", dict(gain_min=1.001)), ("NaN gain_min", dict(gain_min=NAN)),
    ("gain_max < 1", dict(gain_max=0.999)), ("inf gain_max", dict(gain_max=INF)), ("NaN gain_max", dict(gain_max=NAN)),
    ("offset_max < 0", dict(offset_max=-1e-3)), ("inf offset_max", dict(offset_max=INF)),
    ("NaN offset_max", dict(offset_max=NAN)),
    ("min_var < 0", dict(min_var=-1e-9)), ("inf min_var", dict(min_var=INF)), ("NaN min_var", dict(min_var=NAN)),
]
APPLY_REFUSED = [("NULL rgb", dict(rgb=None)), ("NULL params", dict(params=None)), ("NULL out", dict(out=None)),
                 ("width <= 0", dict(width=0)), ("height <= 0", dict(height=-1)),
                 ("2^31 pixels", dict(width=65536, height=32768))]


def refusals():
    """[(function, what, the named arguments over the good ones)] of every refusal of the two entry points."""
    out = [("gsl_map_exposure_estimate", what, dict(GOOD, **over)) for what, over in ESTIMATE_REFUSED]
    return out + [("gsl_map_exposure_apply", what, dict(dict(width=64, height=48), **over)) for what, over in APPLY_REFUSED]


def test_the_prototypes_the_constants_and_the_source(repo_root):
    protos = prototypes(repo_root)
    names = [n for _, n in protos["gsl_map_exposure_estimate"][1]]
    assert names == ["means", "colors", "n_rows", "w2c", "fx", "fy", "cx", "cy", "depth", "intensity", "width", "height",
                     "keep", "beyond", "near_plane", "sat_lo", "sat_hi", "max_residual", "passes", "min_used", "gain_min",
                     "gain_max", "offset_max", "min_var", "sums", "params", "record", "stream"]
    assert protos["gsl_map_exposure_apply"] == ("int", [("const float*", "rgb"), ("int", "width"), ("int", "height"),
                                                        ("const float*", "params"), ("float*", "out"),
                                                        ("void*", "stream")])
    csrc = os.path.join(repo_root, "gsplatloc_amd", "csrc")
    src = open(os.path.join(csrc, "map_exposure.hip")).read()
    for fn in ("gsl_map_exposure_estimate", "gsl_map_exposure_apply", "gsl_map_exposure_values"):
        m = re.search(r'extern "C" \w+ ' + fn + r"\((.*?)\)\s*\{", src, flags=re.S)
        assert m, fn
        defined = [] if m.group(1).strip() == "void" else [
            re.fullmatch(r"\s*(.*?)\s*(\w+)\s*", p, flags=re.S).groups() for p in m.group(1).split(",")]
        assert [(" ".join(t.split()), n) for t, n in defined] == protos[fn][1], fn
    assert "map_exposure.hip" in open(os.path.join(csrc, "Makefile")).read()
    code = src.split("#include", 1)[1]
    assert "#pragma clang fp contract(off)" in code and "atomicAdd(float" not in code and "hipMemset" not in code
    assert "map_project(" in code and "map_inside(" in code and "zero_u32(" in code  # the shared rule, the zeroing launch
    header = open(os.path.join(repo_root, "include", "gsloc_hip.h")).read()
    for name, value in (("VALUES", ref.VALUES), ("RECORD_WORDS", ref.RECORD_WORDS), ("MAX_PASSES", ref.MAX_PASSES),
                        ("OK", ref.OK), ("FEW", ref.FEW), ("FLAT", ref.FLAT), ("RANGE", ref.RANGE)):
        assert int(re.search(r"#define GSL_MAP_EXPOSURE_" + name + r" (\d+)", header).group(1)) == value, name
    assert (mapping.EXPOSURE_VALUES, mapping.EXPOSURE_RECORD_WORDS, mapping.EXPOSURE_MAX_PASSES) == (7, 6, 4)
    assert list(mapping.EXPOSURE_STATUS) == ref.NAMES
    assert _lib.load_library().gsl_map_exposure_values() == ref.VALUES


def test_entry_points_reject_bad_arguments_before_any_launch(repo_root):
    """Every row is refused on the host: the pointers are one dummy HOST buffer, a launch would give GSL_ERR_HIP or
    worse."""
    lib, protos = _lib.load_library(), prototypes(repo_root)
    buf = ctypes.create_string_buffer(b"\x7f" * 1024, 1024)
    seen = set()
    for fn, what, named in refusals():
        params = protos[fn][1]
        pointers = {n: ctypes.addressof(buf) for t, n in params if "*" in t}
        assert set(named) >= {n for t, n in params if "*" not in t}, (fn, what)
        assert call_with(lib, fn, params, named, pointers) == BAD_ARG, (fn, what)
        seen.add(fn)
    assert len(seen) == 2 and buf.raw == b"\x7f" * 1024  # nothing wrote to the buffer


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_the_exposure_kernels_stay_in_registers():
    res = _resources("map_exposure.hip")
    hit = {name: [v for k, v in res.items() if name in k] for name in
           ("k_map_exposure_sums", "k_map_exposure_solve", "k_map_exposure_apply", "k_map_exposure_init")}
    assert all(len(v) == 1 for v in hit.values()), hit
    for name, (r,) in hit.items():
        assert r["ScratchSize"] == 0 and r.get("AGPRs", 0) == 0 and r["Occupancy"] == 8 and r["VGPRs"] <= 32, (name, r)
        assert r["LDS"] == (ref.VALUES * 8 if name == "k_map_exposure_sums" else 0), (name, r)


# ---- (d) MapConfig and the host layer's checks ----------------------------------------------------------------------
def test_map_config_validation():
    c = MapConfig()
    assert (c.photo_exposure, c.exposure_passes, c.exposure_rho, c.exposure_max_residual, c.exposure_saturation,
            c.exposure_min_used, c.exposure_gain, c.exposure_max_offset, c.exposure_min_var) == (
        False, 2, None, 0.1, (0.02, 0.98), 256, (0.5, 2.0), 0.25, 1e-4)
    assert MapConfig(align=True, photo_scale=0.2, photo_exposure=True).photo_exposure is True
    with pytest.raises(ValueError, match="photo_exposure=True needs photo_scale"):
        MapConfig(photo_exposure=True)
    with pytest.raises(ValueError, match="photo_exposure=True needs photo_scale"):
        MapConfig(photo_exposure=True, align=True)
    bad = dict(photo_exposure=[1, None, "yes"], exposure_passes=[0, 5, 2.0, True], exposure_rho=[-0.1, 1.0, NAN, True],
               exposure_max_residual=[-0.1, 1.5, NAN, None], exposure_saturation=[(0.5, 0.5), (-0.1, 0.9), (0.1, 1.1), 0.5,
                                                                                  (0.1, NAN), (0.1, 0.5, 0.9)],
               exposure_min_used=[0, 2.5, True], exposure_gain=[(0.0, 2.0), (1.1, 2.0), (0.5, 0.9), (0.5, INF), None],
               exposure_max_offset=[-0.1, INF, NAN, True], exposure_min_var=[-1e-9, INF, NAN, "0"])
    for field, values in bad.items():
        for v in values:
            with pytest.raises(ValueError, match=field):
                MapConfig(**{field: v})


def test_the_host_layer_checks_its_arguments_and_an_empty_map_launches_nothing():
    w, h = SW, SH
    m = GaussianMap(w, h, MapConfig(align=True, photo_scale=0.2, photo_exposure=True, align_rho=0.1), "cpu")
    depth, rgb, K = torch.full((h, w), 2.0), torch.full((h, w, 3), 100.0), torch.tensor(
        [[8.0, 0.0, 24.0], [0.0, 8.0, 8.0], [0.0, 0.0, 1.0]])
    p = m._exposure_params(None, None, None, None, None, None, None, None)
    assert p == (float(F32(1) - F32(0.1)), float(F32(1) + F32(0.1)), float(F32(0.02)), float(F32(0.98)), float(F32(0.1)),
                 2, 256, 0.5, 2.0, 0.25, 1e-4)  # exposure_rho None: align_rho
    plain = GaussianMap(w, h, MapConfig(), "cpu")
    assert plain._exposure_params(None, None, None, None, None, None, None, None)[0] == float(F32(1) - F32(0.05))
    assert plain._exposure_params(0.25, 0.5, (0.1, 0.9), 4, 7, (0.25, 4.0), 0.5, 0.0) == (
        0.75, 1.25, float(F32(0.1)), float(F32(0.9)), 0.5, 4, 7, 0.25, 4.0, 0.5, 0.0)
    empty = m.estimate_exposure(depth, K, torch.eye(4), NEAR, rgb=rgb)
    assert isinstance(empty, Exposure) and (empty.gain, empty.offset, empty.status, empty.used, empty.seen) == (
        1.0, 0.0, "FEW", 0, 0) and not empty.ok and empty.history == [] and m._exposure is None  # no buffer, no launch
    for bad, match in ((dict(rho=1.0), "rho"), (dict(max_residual=1.5), "max_residual"), (dict(passes=5), "passes"),
                       (dict(passes=0), "passes"), (dict(min_used=0), "min_used"), (dict(gain=(1.5, 2.0)), "exposure_gain"),
                       (dict(saturation=(0.5, 0.2)), "exposure_saturation"), (dict(max_offset=-1.0), "max_offset"),
                       (dict(min_var=NAN), "min_var")):
        with pytest.raises(ValueError, match=match):
            m.estimate_exposure(depth, K, torch.eye(4), NEAR, rgb=rgb, **bad)
    with pytest.raises(ValueError, match="one of the two"):
        m.estimate_exposure(depth, K, torch.eye(4), NEAR)
    with pytest.raises(ValueError, match="one of the two"):
        m.estimate_exposure(depth, K, torch.eye(4), NEAR, rgb=rgb, intensity=torch.zeros(h, w))
    with pytest.raises(ValueError, match="rgb"):
        m.estimate_exposure(depth, K, torch.eye(4), NEAR, rgb=torch.zeros(h, w))
    with pytest.raises(ValueError, match="intensity"):
        m.estimate_exposure(depth, K, torch.eye(4), NEAR, intensity=torch.zeros(h, w + 1))
    with pytest.raises(ValueError, match="rgb"):
        m.apply_exposure(torch.zeros(h, w))
    with pytest.raises(ValueError, match="gain, offset"):
        m.apply_exposure(rgb, (1.0, NAN))
    m.n_live = 3
    for call in (lambda: m.estimate_exposure(depth, K, torch.eye(4), NEAR, intensity=torch.zeros(h, w)),
                 lambda: m.apply_exposure(rgb), lambda: m.apply_exposure(rgb, (1.2, -0.05)),
                 lambda: m.apply_exposure(rgb, Exposure(1.2, -0.05, "OK"))):
        with pytest.raises(AssertionError, match="no CPU path"):
            call()


def test_the_option_of_the_evaluation_driver(tmp_path, capsys):
    from gsplatloc_amd import eval as ev

    with pytest.raises(ValueError, match="map_photo_exposure: an option of map_photo_scale"):
        ev.evaluate_room(None, 200, 3, sequential=True, map_mode=True, map_align=True, map_photo_exposure=True)
    with pytest.raises(SystemExit):
        ev.main(["--root", str(tmp_path), "--sequential", "--map", "--map-align", "--map-photo-exposure"])
    assert "needs --map-photo-scale" in capsys.readouterr().err
