"""The image pyramid and the coarse-to-fine alignment without a GPU: the rule of csrc/map_pyramid.hip on its numpy mirror
(tests/map_pyramid_ref.py), what the feature is for -- the basin of the alignment on a fine-textured wall -- and
everything the library and the host layer decide before a launch.

(a) Depth rule and intrinsics rule together: on the slanted wall the mirror's level-1 .. 3 depths are the float64
    ray-cast depths of the coarse camera at every valid pixel, to 1e-5 relative.
(b) The basin: from the identity, with the truth 0.3 degrees about the optical axis and (t, -0.6 t, 0) metres away, one
    level of 8 steps converges at t = 0.05 (2 pixels) and ends more than 0.02 m off at t = 0.1 and 0.2; levels 3 -> 0 end
    within 2e-4 m and 0.02 degrees at all three, level 0 CONVERGED.  t = 0.3 is beyond three levels.
(c) The entry point's refusals, on the host before any launch; gsl_map_pyramid_floats against the mirror's sizes.
(d) MapConfig, the host layer's checks, the options of the evaluation driver."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from gsplatloc_amd import _lib, mapping
from gsplatloc_amd.mapping import GaussianMap, MapConfig, PoseAlignment, pyramid_intrinsics, pyramid_sizes
from tests import map_align_ref as align
from tests import map_photo_ref as photo
from tests import map_pyramid_ref as ref
from tests.test_kernel_resources import HIPCC, _resources

F32 = np.float32
NEAR = 0.01
KEEP, BEYOND, KAPPA = photo.keep_of(0.05), photo.beyond_of(0.05), F32(1e-3)
SCALE, RMAX = 0.2, 0.1
ALIGN = (8, 1e-3, 7, math.radians(12.8), 0.32, math.radians(1.5e-4), 3e-5)  # MapConfig's defaults
BAD_ARG = -1
FAR, NEAR_T, NEAR_R = 0.02, 2e-4, 0.02  # the issue's conditions: metres off without, metres and degrees with levels


# ---- (a) the depth rule and the intrinsics rule -----------------------------------------------------------------------
def test_coarse_depths_are_the_coarse_cameras_ray_cast_depths():
    d0, _ = ref.fine_wall_frame(np.eye(4), slant=0.2)
    depths, _, intrs = ref.pyramid(d0, 3, KEEP, intr=photo.WALL_INTR)
    for l in (1, 2, 3):
        want = ref.coarse_wall_depth(l, 0.2)
        assert depths[l].shape == want.shape == (photo.WALL_H >> l, photo.WALL_W >> l)
        valid = depths[l] > 0
        assert valid.all()  # a slant of 0.2 is no step: every block is kept
        assert np.abs(depths[l].astype(np.float64)[valid] / want[valid] - 1.0).max() <= 1e-5
    assert intrs[3] == (10.0, 10.0, 9.5, 7.0) and all(isinstance(a, F32) for a in intrs[3])
    assert pyramid_intrinsics(photo.WALL_INTR, 3)[3] == (10.0, 10.0, 9.5, 7.0)
    # ... and a centre that is not dyadic is rounded once per operation, as the mirror does
    odd = (61.3, 59.9, 34.27, 22.61)
    assert pyramid_intrinsics(odd, 4) == [tuple(float(a) for a in lv) for lv in ref.pyramid(
        np.ones((64, 64), F32), 4, KEEP, intr=odd)[2]]


def test_the_rule_on_small_blocks():
    keep = F32(0.9375)
    d = np.array([[2, 2, 4, 4, 1, 1, 2, np.nan], [2, 2, 4, 3.75, 1, 0, 2, 2]], F32)
    assert ref.depth_level(d, keep).tolist() == [[2.0, float(F32(1) / ((F32(.25) + F32(.25) + (F32(.25) + F32(1) / F32(3.75)))
                                                                      * F32(.25))), 0.0, 0.0]]
    d[1, 3] = np.nextafter(F32(3.75), F32(0))  # one step beyond the bound: a depth step
    assert ref.depth_level(d, keep)[0, 1] == 0.0
    y = np.array([[0.25, 0.5, np.nan, 0, 3], [0.75, 1.0, 0, 0, 3], [9, 9, 9, 9, 9]], F32)
    out = ref.intensity_level(y)  # the odd last column and row are dropped
    assert out.shape == (1, 2) and out[0, 0] == 0.625 and np.isnan(out[0, 1])


# ---- (b) the basin ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def basin():
    """Per t: (one level's error, its last status, the levels' error, level 0's history column of statuses, the steps
    every level applied)."""
    out = {}
    start = np.eye(4, dtype=F32)
    for t in (0.05, 0.1, 0.2, 0.3):
        c = ref.fine_wall_case(t)
        args = (c["means"], c["colors"], start, c["intr"], c["depth"], c["image"], KEEP, BEYOND, KAPPA, NEAR, SCALE, RMAX)
        one = photo.pose_align(*args, *ALIGN)
        lv = ref.pose_align(*args, *ALIGN, levels=3)
        out[t] = (photo.pose_error(one[0], c["truth"]), int(one[4][-1, 0]), photo.pose_error(lv[-1][0], c["truth"]),
                  lv[-1][4][:, 0].tolist(), [r[2] for r in lv])
    return out


def test_one_level_converges_from_two_pixels_and_not_from_four(basin, capsys):
    with capsys.disabled():
        for t, (e1, s1, e3, h3, n3) in basin.items():
            print(f"\nt = {t:.2f} m: one level {e1[0]:.3e} m {e1[1]:.4f} deg ({align.NAMES[s1]}); levels 3 -> 0 "
                  f"{e3[0]:.3e} m {e3[1]:.4f} deg, steps per level {n3}", end="")
    (e1, s1, _, _, _) = basin[0.05]
    assert e1[0] <= NEAR_T and e1[1] <= NEAR_R and s1 == align.CONVERGED
    for t in (0.1, 0.2):
        assert basin[t][0][0] > FAR and basin[t][1] != align.CONVERGED, t


def test_three_levels_converge_from_eight_pixels(basin):
    for t in (0.05, 0.1, 0.2):
        _, _, e3, h3, n3 = basin[t]
        assert e3[0] <= NEAR_T and e3[1] <= NEAR_R, (t, e3)
        assert h3[-1] == align.CONVERGED and h3.index(align.CONVERGED) <= 3, (t, h3)  # level 0 has little left to do
        assert len(n3) == 4
    # twelve pixels are beyond three levels: not claimed, and said so
    assert basin[0.3][2][0] > FAR


def test_the_levels_go_on_from_the_working_pose_and_a_refusal_leaves_it():
    c = ref.fine_wall_case(0.1)
    start = np.eye(4, dtype=F32)
    args = (c["means"], c["colors"], start, c["intr"], c["depth"], c["image"], KEEP, BEYOND, KAPPA, NEAR, SCALE, RMAX)
    lv = ref.pose_align(*args, *ALIGN, levels=2, level_steps=3)
    assert [len(r[4]) for r in lv] == [3, 3, 8]
    depths, images, intrs = ref.pyramid(c["depth"], 2, KEEP, c["image"], c["intr"])
    for l, a, b in zip((1, 0), lv, lv[1:]):  # a level is the single-level mirror started at the work before it
        alone = photo.pose_align(c["means"], c["colors"], a[1], intrs[l], depths[l], images[l], KEEP, BEYOND, KAPPA, NEAR,
                                 SCALE, RMAX, len(b[4]), *ALIGN[1:])
        assert np.array_equal(alone[0], b[0]) and np.array_equal(alone[4], b[4])
    # a slanted wall under pyramid_rho = 0: no block has four equal depths, the coarse levels are empty -- FEW there, the
    # pose unmoved -- and level 0 is the single-level alignment from the start, bit for bit
    s = ref.fine_wall_case(0.05, slant=0.2)
    sargs = (s["means"], s["colors"], start, s["intr"], s["depth"], s["image"], KEEP, BEYOND, KAPPA, NEAR, SCALE, RMAX)
    few = ref.pose_align(*sargs, *ALIGN, levels=2, keep_p=F32(1.0))
    for r in few[:2]:
        assert (r[4][:, 0] == align.FEW).all() and r[2] == 0 and np.array_equal(r[1], start)
    alone = photo.pose_align(*sargs, *ALIGN)
    assert few[2][2] > 0 and np.array_equal(few[2][0], alone[0]) and np.array_equal(few[2][4], alone[4])
    # the geometric alignment takes levels as well (image None)
    geo = ref.pose_align(c["means"], None, start, c["intr"], c["depth"], None, KEEP, BEYOND, KAPPA, NEAR, 0, 0, *ALIGN,
                         levels=2)
    assert len(geo) == 3 and all(len(r) == 7 for r in geo)
    batch = ref.pose_align_batch(c["means"], c["colors"], [start, start], *args[3:], *ALIGN, levels=2, level_steps=3)
    assert len(batch) == 2 and np.array_equal(batch[0][-1][0], lv[-1][0]) and batch[0][-1][3] in (0, 1, 2)


# ---- (c) the entry point ----------------------------------------------------------------------------------------------
REFUSED = [("NULL depth", dict(depth=None)), ("NULL depth_out", dict(depth_out=None)),
           ("intensity without intensity_out", dict(intensity_out=None)),
           ("intensity_out without intensity", dict(intensity=None)), ("width <= 0", dict(width=0)),
           ("height <= 0", dict(height=-3)), ("2^31 pixels", dict(width=65536, height=32768)),
           ("levels == 0", dict(levels=0)), ("levels == 5", dict(levels=5)), ("levels < 0", dict(levels=-1)),
           ("keep == 0", dict(keep=0.0)), ("keep > 1", dict(keep=1.5)), ("keep NaN", dict(keep=float("nan"))),
           ("keep < 0", dict(keep=-0.5)), ("coarsest 3 wide", dict(width=15, levels=2)),
           ("coarsest 3 high", dict(height=31, levels=3)), ("coarsest 2 x 2", dict(width=32, height=32, levels=4))]


def test_the_entry_point_refuses_bad_arguments_before_any_launch():
    """The pointers are one dummy HOST buffer: a launch would fault or give GSL_ERR_HIP."""
    lib = _lib.load_library()
    buf = ctypes.create_string_buffer(b"\x7f" * 1024, 1024)
    at = ctypes.addressof(buf)
    good = dict(depth=at, intensity=at, width=64, height=48, levels=2, keep=0.95, depth_out=at, intensity_out=at)
    for what, over in REFUSED:
        a = dict(good, **over)
        assert lib.gsl_map_pyramid(a["depth"], a["intensity"], a["width"], a["height"], a["levels"], a["keep"],
                                   a["depth_out"], a["intensity_out"], None) == BAD_ARG, what
        if set(over) <= {"width", "height", "levels"}:
            assert lib.gsl_map_pyramid_floats(a["width"], a["height"], a["levels"]) == 0, what
    assert buf.raw == b"\x7f" * 1024


def test_the_floats_of_a_pyramid():
    lib = _lib.load_library()
    assert lib.gsl_map_pyramid_floats(160, 120, 3) == 80 * 60 + 40 * 30 + 20 * 15
    for w, h in ((160, 120), (37, 29), (70, 45), (33, 36), (64, 64), (640, 480), (16, 16), (17, 1000), (1279, 721)):
        for levels in range(0, 6):
            want = ref.floats(w, h, levels)
            assert lib.gsl_map_pyramid_floats(w, h, levels) == want, (w, h, levels)
            if want:
                assert pyramid_sizes(w, h, levels) == [(w, h)] + ref.sizes(w, h, levels)
                assert want <= (w * h) // 3  # at most a third of the frame is written
            else:
                with pytest.raises(ValueError, match="levels"):
                    pyramid_sizes(w, h, levels)
    assert lib.gsl_map_pyramid_floats(64, 64, 4) == 32 * 32 + 16 * 16 + 8 * 8 + 4 * 4
    assert mapping.PYRAMID_MAX_LEVELS == ref.MAX_LEVELS == 4 and mapping.PYRAMID_MIN_SIDE == ref.MIN_SIDE


def test_the_source_keeps_to_its_rules(repo_root):
    csrc = os.path.join(repo_root, "gsplatloc_amd", "csrc")
    src = open(os.path.join(csrc, "map_pyramid.hip")).read()
    assert "map_pyramid.hip" in open(os.path.join(csrc, "Makefile")).read()
    assert "#pragma clang fp contract(off)" in src and "atomic" not in src.split("#include", 1)[1]
    assert "hipMemset" not in src and "zero_u32" not in src
    header = open(os.path.join(repo_root, "include", "gsloc_hip.h")).read()
    assert "#define GSL_MAP_PYRAMID_MAX_LEVELS 4" in header


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_the_pyramid_kernel_needs_next_to_nothing():
    """Both instantiations: no scratch, the tile's levels 1 .. 3 in LDS (336 floats per image), full occupancy."""
    res = {k: v for k, v in _resources("map_pyramid.hip").items() if "k_map_pyramid" in k}
    assert len(res) == 2
    assert sorted(r["LDS"] for r in res.values()) == [336 * 4, 2 * 336 * 4]
    for r in res.values():
        assert r["ScratchSize"] == 0 and r["AGPRs"] == 0 and r["VGPRs"] <= 64 and r["Occupancy"] == 8, r


# ---- (d) MapConfig, the host layer, the evaluation driver ---------------------------------------------------------------
def test_map_config_validation():
    c = MapConfig()
    assert (c.align_levels, c.align_level_steps, c.pyramid_rho) == (0, None, None)
    assert MapConfig(align=True, align_levels=3, align_level_steps=4, pyramid_rho=0.1).align_levels == 3
    assert MapConfig(loop=True, origins=True, align_levels=4).align_levels == 4
    assert MapConfig(align_level_steps=2, pyramid_rho=0.0).pyramid_rho == 0.0  # without levels they are only numbers
    with pytest.raises(ValueError, match="align_levels needs align=True or loop=True"):
        MapConfig(align_levels=2)
    with pytest.raises(ValueError, match="align_levels needs"):
        MapConfig(align_levels=2, info=True, reloc=True)
    bad = dict(align_levels=[-1, 5, 1.0, True, None, "2"], align_level_steps=[0, 33, 2.0, True, "4"],
               pyramid_rho=[-0.1, 1.0, float("nan"), True, "0.05"])
    for field, values in bad.items():
        for v in values:
            with pytest.raises(ValueError, match=field):
                MapConfig(align=True, **{field: v})


def test_the_host_layer_checks_its_arguments():
    w, h = 64, 48
    m = GaussianMap(w, h, MapConfig(align=True), "cpu")
    depth, K, eye = torch.ones(h, w), torch.tensor([[50.0, 0, 31.5], [0, 50.0, 23.5], [0, 0, 1]]), torch.eye(4)
    for bad in (-1, 5, 1.5, True, "2"):
        with pytest.raises(ValueError, match="levels"):
            m.align_pose(depth, K, eye, NEAR, levels=bad)
        with pytest.raises(ValueError, match="levels"):
            m.align_poses(depth, K, [eye], NEAR, levels=bad)
    with pytest.raises(ValueError, match="smaller than 4 x 4"):
        m.align_pose(depth, K, eye, NEAR, levels=4)  # 64 x 48 -> 4 x 3
    for bad in (0, 33, 1.5, True):
        with pytest.raises(ValueError, match="level_steps"):
            m.align_pose(depth, K, eye, NEAR, levels=2, level_steps=bad)
    for bad in (0, 5, None, 2.0):
        with pytest.raises(ValueError, match="levels"):
            m.pyramid(depth, bad)
    with pytest.raises(ValueError, match="rho"):
        m.pyramid(depth, 2, rho=1.0)
    with pytest.raises(ValueError, match="depth"):
        m.pyramid(torch.ones(h, w + 1), 2)
    with pytest.raises(ValueError, match="intensity"):
        m.pyramid(depth, 2, intensity=torch.ones(h + 1, w))
    # the keep of a pyramid: the argument, then pyramid_rho, then the alignment's rho
    assert m._pyramid_keep(0.1) == float(F32(1) - F32(0.1))
    assert m._pyramid_keep(None, 0.2) == float(F32(1) - F32(0.2))
    assert m._pyramid_keep(None) == float(F32(1) - F32(m.cfg.depth_rho))
    assert GaussianMap(w, h, MapConfig(align=True, align_rho=0.3), "cpu")._pyramid_keep(None) == float(F32(1) - F32(0.3))
    assert GaussianMap(w, h, MapConfig(align=True, pyramid_rho=0.25), "cpu")._pyramid_keep(None, 0.2) == 0.75
    # the defaults come from the configuration; an empty map answers without a launch, levels or not
    cfg = GaussianMap(w, h, MapConfig(align=True, align_levels=3, align_level_steps=5), "cpu")
    assert cfg._levels_params(None, None, 8) == (3, 5) and cfg._levels_params(0, 2, 8) == (0, 2)
    assert m._levels_params(None, None, 8) == (0, 8) and m._levels_params(2, None, 6) == (2, 6)
    empty = cfg.align_pose(depth, K, eye, NEAR)
    assert empty.status == "FEW" and empty.level_history is None and empty.level_steps is None
    assert [a.status for a in cfg.align_poses(depth, K, [eye, eye], NEAR)] == ["FEW", "FEW"]
    fields = [f for f in PoseAlignment.__dataclass_fields__]
    assert fields[:9] == ["c2w", "w2c64", "status", "steps", "used", "tested", "history", "closed", "final"]
    assert fields[9:] == ["level_history", "level_steps"]  # the fields of before, in their order
    cfg.n_live = 3
    for call in (lambda: cfg.pyramid(depth, 2), lambda: cfg.align_pose(depth, K, eye, NEAR),
                 lambda: cfg.align_poses(depth, K, [eye], NEAR)):
        with pytest.raises(AssertionError, match="no CPU path"):
            call()
    # a prebuilt pyramid has to be this frame's, deep enough, and hold intensities for a photometric call
    from gsplatloc_amd.mapping import FramePyramid

    short = FramePyramid(1, [depth, depth[:24, :32]], None, [(w, h), (32, 24)], 0.95)
    with pytest.raises(ValueError, match="at least 2 levels"):
        cfg._level_frames(depth, (50.0, 50.0, 31.5, 23.5), None, 2, short, 0.95)
    with pytest.raises(ValueError, match="holds no intensities"):
        cfg._level_frames(depth, (50.0, 50.0, 31.5, 23.5), (depth, 0.2, 0.1), 1, short, 0.95)
    frames = cfg._level_frames(depth, (50.0, 50.0, 31.5, 23.5), None, 1, short, 0.95)
    assert [f[1] for f in frames] == [(32, 24), (w, h)] and frames[0][2] == (25.0, 25.0, 15.5, 11.5)
    assert frames[1][0] is depth and frames[0][3] is None


def test_the_options_of_the_evaluation_driver(tmp_path):
    from gsplatloc_amd import eval as ev

    with pytest.raises(ValueError, match="map_align_levels belongs to the map mode"):
        ev.evaluate_room(None, 200, 3, sequential=True, map_align_levels=2)
    with pytest.raises(ValueError, match="map_align or map_loop"):
        ev.evaluate_room(None, 200, 3, sequential=True, map_mode=True, map_align_levels=2)
    with pytest.raises(ValueError, match="map_align_level_steps"):
        ev.evaluate_room(None, 200, 3, sequential=True, map_mode=True, map_align=True, map_align_level_steps=4)
    for extra, word in ((["--sequential", "--map", "--map-align-levels", "2"], "needs --map-align"),
                        (["--sequential", "--map", "--map-align", "--map-align-level-steps", "4"],
                         "needs --map-align-levels")):
        with pytest.raises(SystemExit):
            ev.main(["--root", str(tmp_path)] + extra)
