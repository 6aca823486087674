"""Pose alignment (csrc/map_align.hip, GaussianMap.align_pose, MapConfig.align), the parts that need no GPU: the numpy
mirror tests/map_align_ref.py -- tests/map_info_ref.py per iteration, then the float64 step in the device's order -- on
the corner view of tests/test_map_info_cpu.py, where a start 6.4 cm / 3 degrees off must converge onto the query's pose,
on one plane, where three directions are open and must not move, and on the inputs every refusal answers; MapConfig;
the entry point against its prototype and its argument checks; the step kernel's budget; and Localizer(mode="map") with
``align`` around the stand-ins of tests/test_map_score_cpu.py and a map whose device calls are the mirrors.

The corner view (160x120, gsplatloc_amd.synthetic.room_depth): the map is the back-projection of one frame at position
(0.6, 0.1, 0.8), yaw 35 degrees about y; the query frame is taken at (0.65, 0.1, 0.76), yaw 38 -- 6.4 cm and 3 degrees
away -- and the alignment starts at the map's pose, with the defaults of MapConfig.  The float64 prototype of this
set-up reached 1.3e-6 m / 2.6e-5 degrees after 7 steps; the bounds are 1e-4 m and 1e-3 degrees, about three times the
stop tolerance of a step (3e-5 m, 1.5e-4 degrees) and below the tracker's smallest recorded frame error (3.6e-4 m).
What the mirror measures is printed (NOTES.md, "Pose alignment")."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from gsplatloc_amd import _lib, mapping
from gsplatloc_amd.localizer import LocalizeResult
from gsplatloc_amd.mapping import MapConfig, PoseAlignment
from gsplatloc_amd.synthetic import replica_intrinsics, room_depth
from tests import map_align_ref as ref
from tests import map_info_ref as info
from tests import test_map_cpu as base
from tests import test_map_info_cpu as tinfo
from tests import test_map_score_cpu as score
from tests.test_abi import prototypes
from tests.test_kernel_resources import HIPCC, _resources

F32 = np.float32
NEAR = tinfo.NEAR
KEEP, BEYOND, KAPPA = info.keep_of(0.05), info.beyond_of(0.05), F32(1e-3)
DEFAULTS = dict(max_steps=8, damping=1e-3, min_used=7, max_rot=math.radians(12.8), max_trans=0.32,
                eps_rot=math.radians(1.5e-4), eps_trans=3e-5)
CW, CH = tinfo.CW, tinfo.CH
AT_MAP = tinfo.yaw_pose((0.6, 0.1, 0.8), 35.0)
QUERIES = {"5cm3deg": tinfo.yaw_pose((0.65, 0.1, 0.76), 38.0), "1cm0.5deg": tinfo.yaw_pose((0.608, 0.1, 0.794), 35.5)}


def align(means, start_c2w, intr, depth, **over):
    a = dict(DEFAULTS, **over)
    return ref.pose_align(means, info.w2c_of(start_c2w), intr, depth, KEEP, BEYOND, KAPPA, NEAR, a["max_steps"],
                          a["damping"], a["min_used"], a["max_rot"], a["max_trans"], a["eps_rot"], a["eps_trans"])


def errors(P, truth_c2w):
    """(metres, degrees) between the camera-to-world pose of the world-to-camera P [3,4] float64 and the truth; the
    angle from |R - R_truth|_F^2 = 8 sin^2(theta / 2), which resolves what acos((trace - 1) / 2) cannot."""
    c2w = np.linalg.inv(np.vstack([P, [0.0, 0.0, 0.0, 1.0]]))
    d = c2w[:3, :3] - truth_c2w[:3, :3]
    return (float(np.linalg.norm(c2w[:3, 3] - truth_c2w[:3, 3])),
            math.degrees(2.0 * math.asin(min(1.0, math.sqrt(float((d * d).sum()) * 0.125)))))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def corner():
    K = replica_intrinsics(CW, CH)
    intr = tinfo.intrinsics(K)
    d_map = room_depth(CW, CH, K, torch.from_numpy(AT_MAP).float()).numpy()
    depths = {k: room_depth(CW, CH, K, torch.from_numpy(q).float()).numpy() for k, q in QUERIES.items()}
    return dict(intr=intr, means=tinfo.back_projection(d_map, intr, AT_MAP), depths=depths)


# ---- the corner view ------------------------------------------------------------------------------------------------
def test_a_start_five_centimetres_off_converges_in_the_corner(corner, capsys):
    truth = QUERIES["5cm3deg"]
    P, work, taken, done, rows, xis, _ = align(corner["means"], AT_MAP, corner["intr"], corner["depths"]["5cm3deg"])
    before = errors(info.w2c_of(AT_MAP)[:3].astype(np.float64), truth)
    eT, eR = errors(P, truth)
    with capsys.disabled():
        print(f"[align] corner 5 cm / 3 deg: {before[0]:.3e} m {before[1]:.3e} deg -> {eT:.3e} m {eR:.3e} deg after "
              f"{taken} steps, statuses {[ref.NAMES[s] for s in rows[:, 0]]}, used {rows[:, 1].tolist()}, |upsilon| "
              f"{[float(f'{np.linalg.norm(x[3:]):.2e}') for x in xis]}")
    assert 0.06 < before[0] < 0.07 and 2.9 < before[1] < 3.1
    assert rows[-1, 0] == ref.CONVERGED and done == 1 and 1 <= taken <= 8
    first = rows[:, 0].tolist().index(ref.CONVERGED)
    assert taken == first + 1 and all(s == ref.STEPPED for s in rows[:first, 0])
    assert all(s == ref.CONVERGED for s in rows[first:, 0]) and not xis[first + 1:].any()
    assert eT <= 1e-4 and eR <= 1e-3, (eT, eR)
    assert same_bits(work[:3], P.astype(F32)) and work[3].tolist() == [0.0, 0.0, 0.0, 1.0]
    assert (rows[:, 1] > 10000).all() and (rows[:, 1] <= rows[:, 2]).all()


def test_a_start_one_centimetre_off_converges_in_four_steps(corner, capsys):
    truth = QUERIES["1cm0.5deg"]
    P, _, taken, done, rows, _, _ = align(corner["means"], AT_MAP, corner["intr"], corner["depths"]["1cm0.5deg"])
    eT, eR = errors(P, truth)
    with capsys.disabled():
        print(f"[align] corner 1 cm / 0.5 deg: {eT:.3e} m {eR:.3e} deg after {taken} steps")
    assert rows[-1, 0] == ref.CONVERGED and taken <= 4 and eT <= 1e-4 and eR <= 1e-3


def test_one_step_is_the_solution_of_the_damped_normal_equations(corner):
    """The LDL^T of the mirror against numpy's solver, and the Cayley map against the exponential to first order."""
    sums = info.pose_info(corner["means"], info.w2c_of(AT_MAP), corner["intr"], corner["depths"]["5cm3deg"], KEEP,
                          BEYOND, KAPPA, NEAR)
    H, g, _, used, _ = info.unpack(sums)
    x = ref.solve(sums, 1e-3)
    assert np.allclose(x, -np.linalg.solve(H + 1e-3 * used * np.eye(6), g), rtol=1e-9, atol=1e-15)
    omega = np.array([0.02, -0.05, 0.03])
    R = ref.cayley(omega)
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-15) and abs(np.linalg.det(R) - 1.0) < 1e-15
    angle = math.acos((np.trace(R) - 1.0) / 2.0)
    assert abs(angle - 2.0 * math.atan(np.linalg.norm(omega) / 2.0)) < 1e-12  # about omega, by 2 atan(|omega| / 2)
    assert np.allclose(R @ omega, omega, atol=1e-16)
    tiny = 1e-7 * omega
    skew = np.array([[0.0, -tiny[2], tiny[1]], [tiny[2], 0.0, -tiny[0]], [-tiny[1], tiny[0], 0.0]])
    assert np.allclose(ref.cayley(tiny), np.eye(3) + skew, atol=1e-15)
    assert same_bits(ref.cayley(np.zeros(3)), np.eye(3))  # the fixed point: no step, no move


# ---- one plane ------------------------------------------------------------------------------------------------------
def test_one_plane_moves_along_its_normal_only():
    depth, means = tinfo.plane_case()
    query = np.full_like(depth, 2.02)
    P, work, taken, done, rows, xis, _ = align(means, np.eye(4), tinfo.PINTR, query)
    assert taken >= 1 and rows[-1, 0] in (ref.CONVERGED, ref.STEPPED)
    assert (rows[:, 1] == (tinfo.PW - 2) * (tinfo.PH - 2)).all()
    # n = (0, 0, 1) exactly: the sums of omega_z, upsilon_x and upsilon_y are exact zeros, and so are their steps
    assert not xis[:, 2].any() and not xis[:, 3].any() and not xis[:, 4].any() and xis[0, 5] > 0.019
    assert abs(P[2, 3] - 0.02) <= 1e-4 and abs(P[0, 3]) <= 1e-4 and abs(P[1, 3]) <= 1e-4, P
    assert np.allclose(P[:, :3], np.eye(3), atol=1e-4)


def test_one_plane_without_damping_is_singular():
    depth, means = tinfo.plane_case()
    query = np.full_like(depth, 2.02)
    P, work, taken, done, rows, xis, _ = align(means, np.eye(4), tinfo.PINTR, query, damping=0.0)
    assert (rows[:, 0] == ref.SINGULAR).all() and taken == 0 and done == 1 and not xis.any()
    assert same_bits(P, np.eye(4)[:3]) and same_bits(work, np.eye(4, dtype=F32))


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_six_rows_are_too_few():
    depth, means = tinfo.plane_case()
    centre = (tinfo.PH // 2) * tinfo.PW + tinfo.PW // 2
    six = means[centre - 3:centre + 3]
    start = tinfo.yaw_pose((0.001, 0.0, 0.002), 0.1)
    P, work, taken, done, rows, xis, sums = align(six, start, tinfo.PINTR, depth)
    assert sums[28] == 6 and (rows[:, 0] == ref.FEW).all() and (rows[:, 1] == 6).all() and taken == 0 and done == 1
    assert same_bits(work, info.w2c_of(start)) and same_bits(P, info.w2c_of(start)[:3].astype(np.float64))
    seven = means[centre - 3:centre + 4]
    assert align(seven, start, tinfo.PINTR, depth)[4][0, 0] != ref.FEW
    assert (align(seven, start, tinfo.PINTR, depth, min_used=8)[4][:, 0] == ref.FEW).all()


def test_a_step_beyond_the_bound_is_not_taken(corner):
    P, work, taken, done, rows, xis, _ = align(corner["means"], AT_MAP, corner["intr"], corner["depths"]["5cm3deg"],
                                               max_trans=1e-3)
    assert (rows[:, 0] == ref.TOO_FAR).all() and taken == 0 and done == 1
    assert np.linalg.norm(xis[0, 3:]) > 1e-3 and not xis[1:].any()  # the refused step is on record, at step 0
    assert same_bits(work, info.w2c_of(AT_MAP)) and same_bits(P, info.w2c_of(AT_MAP)[:3].astype(np.float64))
    rot = align(corner["means"], AT_MAP, corner["intr"], corner["depths"]["5cm3deg"], max_rot=math.radians(0.1))
    assert (rot[4][:, 0] == ref.TOO_FAR).all() and same_bits(rot[1], info.w2c_of(AT_MAP))


# ---- MapConfig ------------------------------------------------------------------------------------------------------
def test_map_config_validation():
    c = MapConfig()
    assert (c.align, c.align_steps, c.align_damping, c.align_rho) == (False, 8, mapping.INFO_MIN_EIG, None)
    assert (c.align_max_rot_deg, c.align_max_trans, c.align_eps_rot_deg, c.align_eps_trans) == (12.8, 0.32, 1.5e-4, 3e-5)
    ok = MapConfig(align=True, align_steps=32, align_damping=0.0, align_rho=0.0, align_eps_rot_deg=0.0, align_eps_trans=0)
    assert ok.align and MapConfig(align=True, align_steps=1).align_steps == 1
    bad = dict(align=[1, "yes", None, 0.5],
               align_steps=[0, 33, -1, 8.0, True, None, "8"],
               align_damping=[-1e-3, float("inf"), float("nan"), True, None, "1e-3"],
               align_rho=[1.0, -0.01, float("nan"), True, "0.05"],
               align_max_rot_deg=[0.0, -1.0, float("inf"), float("nan"), True, None],
               align_max_trans=[0.0, -1.0, float("inf"), float("nan"), True, None],
               align_eps_rot_deg=[-1e-9, float("inf"), float("nan"), True, None],
               align_eps_trans=[-1e-9, float("inf"), float("nan"), True, None])
    for field, values in bad.items():
        for v in values:
            with pytest.raises(ValueError, match=field):
                MapConfig(**{field: v})
    for rho in (1.0, -0.01):
        with pytest.raises(ValueError, match="depth_rho"):
            MapConfig(align=True, depth_rho=rho)
        assert MapConfig(align=True, depth_rho=rho, align_rho=0.05).align
        assert MapConfig(depth_rho=rho).depth_rho == rho  # only the option needs it


# ---- the entry point ------------------------------------------------------------------------------------------------
BAD_ARG = -1
FN = "gsl_map_pose_align"
GOOD = dict(tinfo.GOOD, max_steps=8, damping=1e-3, min_used=7, max_rot=0.2, max_trans=0.3, eps_rot=1e-6, eps_trans=1e-5)
REFUSED = [(what, over) for what, over in tinfo.REFUSED if "out" not in over] + [
    ("NULL sums", dict(sums=None)), ("NULL work", dict(work=None)), ("NULL state", dict(state=None)),
    ("NULL history", dict(history=None)), ("max_steps == 0", dict(max_steps=0)), ("max_steps == 33", dict(max_steps=33)),
    ("max_steps < 0", dict(max_steps=-1)), ("damping < 0", dict(damping=-1e-3)), ("NaN damping", dict(damping=float("nan"))),
    ("inf damping", dict(damping=float("inf"))), ("min_used == 6", dict(min_used=6)), ("min_used < 0", dict(min_used=-7)),
    ("max_rot == 0", dict(max_rot=0.0)), ("NaN max_rot", dict(max_rot=float("nan"))),
    ("max_trans == 0", dict(max_trans=0.0)), ("inf max_trans", dict(max_trans=float("inf"))),
    ("eps_rot < 0", dict(eps_rot=-1e-9)), ("NaN eps_trans", dict(eps_trans=float("nan"))),
]


def call_with(lib, params, named, pointers):
    """gsl_map_pose_align with the named arguments over GOOD; ``pointers``: parameter name -> address."""
    args = []
    for c_type, name in params:
        if name == "stream":
            args.append(None)
        elif name in named:
            args.append(named[name])
        else:
            args.append(pointers[name] if "*" in c_type else 0)
    return getattr(lib, FN)(*args)


def test_header_binding_and_definition_agree(repo_root):
    ret, params = prototypes(repo_root)[FN]
    info_params = prototypes(repo_root)["gsl_map_pose_info"][1]
    assert ret == "int" and [n for _, n in params] == [n for _, n in info_params[:-2]] + [
        "max_steps", "damping", "min_used", "max_rot", "max_trans", "eps_rot", "eps_trans", "sums", "work", "state",
        "history", "stream"]
    assert params[:len(info_params) - 2] == info_params[:-2]  # the arguments of gsl_map_pose_info, as they are there
    types = dict((n, t) for t, n in params)
    assert (types["sums"], types["work"], types["damping"], types["w2c"]) == ("int64_t*", "float*", "double", "const float*")
    assert len(_lib._SIGNATURES[FN][1]) == len(params)
    csrc = os.path.join(repo_root, "gsplatloc_amd", "csrc")
    src = open(os.path.join(csrc, "map_align.hip")).read()
    m = re.search(r'extern "C" int gsl_map_pose_align\((.*?)\)\s*\{', src, flags=re.S)
    assert m, "no definition of gsl_map_pose_align"
    defined = [re.fullmatch(r"\s*(.*?)\s*(\w+)\s*", p, flags=re.S).groups() for p in m.group(1).split(",")]
    assert [(" ".join(t.split()), n) for t, n in defined] == params
    header = open(os.path.join(repo_root, "include", "gsloc_hip.h")).read()
    define = lambda name: int(re.search(rf"#define {name} (\d+)", header).group(1))  # noqa: E731
    lib = _lib.load_library()
    assert define("GSL_MAP_ALIGN_MAX_STEPS") == 32 == mapping.ALIGN_MAX_STEPS == ref.MAX_STEPS == lib.gsl_map_align_max_steps()
    assert define("GSL_MAP_ALIGN_STATE_WORDS") == mapping.ALIGN_STATE_WORDS == 14
    assert define("GSL_MAP_ALIGN_ROW_WORDS") == mapping.ALIGN_ROW_WORDS == 10
    for code, name in enumerate(ref.NAMES):
        assert define(f"GSL_MAP_ALIGN_{name}") == code and mapping.ALIGN_STATUS[code] == name
    assert "map_align.hip" in open(os.path.join(csrc, "Makefile")).read()
    assert "#pragma clang fp contract(off)" in src and "asm" not in re.sub(r"//.*", "", src)
    # one copy of the sums' launch: both entry points go through the internal launcher, which is no C symbol
    assert src.count("gsl::map_pose_info_launch(") == 1 and "k_map_pose_info" not in re.sub(r"//.*", "", src)
    info_src = open(os.path.join(csrc, "map_info.hip")).read()
    assert info_src.count("hipLaunchKernelGGL(") == 1 and info_src.count("map_pose_info_launch(") == 2
    assert "map_pose_info_launch(" in open(os.path.join(csrc, "gsloc_internal.h")).read()


def test_entry_point_rejects_bad_arguments_before_any_launch(repo_root):
    """Every row is refused on the host: the pointers are one dummy HOST buffer, a launch would give GSL_ERR_HIP or
    worse."""
    lib = _lib.load_library()
    params = prototypes(repo_root)[FN][1]
    buf = ctypes.create_string_buffer(b"\x7f" * 4096, 4096)
    pointers = {n: ctypes.addressof(buf) for t, n in params if "*" in t}
    assert len(REFUSED) == len(tinfo.REFUSED) - 1 + 18
    for what, over in REFUSED:
        named = dict(GOOD, **over)
        assert set(named) <= {n for _, n in params}, what
        assert call_with(lib, params, named, pointers) == BAD_ARG, what
    assert buf.raw == b"\x7f" * 4096  # nothing wrote to the buffer


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_the_step_kernel_stays_in_registers():
    """k_map_align_step: the 6 x 6 factorisation of one lane, every loop unrolled -- no scratch and no LDS."""
    res = _resources("map_align.hip")
    hit = [v for k, v in res.items() if "k_map_align_step" in k]
    assert len(hit) == 1 and hit[0]["ScratchSize"] == 0 and hit[0]["LDS"] == 0 and hit[0]["AGPRs"] == 0, hit
    init = [v for k, v in res.items() if "k_map_align_init" in k]
    assert len(init) == 1 and init[0]["ScratchSize"] == 0 and init[0]["LDS"] == 0, init


# ---- GaussianMap.align_pose and Localizer(mode="map", align) around the mirrors -------------------------------------
W, H = base.W, base.H
CFG_NEAR = score.CFG_NEAR


class _AlignMirrorMap(tinfo._InfoMirrorMap):
    """The stand-in map of tests/test_map_info_cpu.py with the mirror of csrc/map_align.hip; one log for all calls."""

    def _align_launch(self, depth, intr, w2c, keep, beyond, kappa, near, steps, damping, min_used, max_rot, max_trans,
                      eps_rot, eps_trans):
        P, work, taken, _, rows, xis, _ = ref.pose_align(
            self.means[:self.n_live].numpy(), w2c.numpy(), intr, depth.numpy(), F32(keep), F32(beyond), F32(kappa), near,
            steps, damping, min_used, max_rot, max_trans, eps_rot, eps_trans)
        score._ScoreMirrorMap.log.append(dict(call="align", w2c=w2c.numpy().copy(), depth=depth.clone(), near=near,
                                              rows=self.n_live, keep=keep, beyond=beyond, kappa=kappa, steps=steps,
                                              damping=damping, min_used=min_used, bounds=(max_rot, max_trans),
                                              eps=(eps_rot, eps_trans), pose=P.copy(), taken=taken, history=rows.copy()))
        return P, work, taken, rows, xis


class _WorseMap(_AlignMirrorMap):
    """... whose scores say that the second of two poses sees through one row more than the first."""

    def _score_launch(self, depth, intr, w2c, near):
        counts = super()._score_launch(depth, intr, w2c, near)
        if len(counts) == 2:
            counts[1] = counts[0] + np.array([0, -1, 1])
        return counts


class _FewerRowsMap(_AlignMirrorMap):
    """... whose scores say that the second of two poses has lost ten rows over the image's edge, all of which agreed."""

    def _score_launch(self, depth, intr, w2c, near):
        counts = super()._score_launch(depth, intr, w2c, near)
        if len(counts) == 2:
            counts[1] = counts[0] - np.array([10, 10, 0])
        return counts


def _localizer(monkeypatch, factory=_AlignMirrorMap, **cfg):
    import gsplatloc_amd.data.dataset as DS
    from gsplatloc_amd.localizer import Localizer
    from gsplatloc_amd.my_gsplat import TrackerConfig

    monkeypatch.setattr(DS, "compute_depth_gt", lambda pts, col, Ks, c2w, height, width: torch.zeros(height, width))
    score._StartTracker.made = base._Tracker.made = []
    loc = Localizer(replica_intrinsics(W, H), W, H, TrackerConfig(max_steps=5), normalize=False, motion="hold",
                    device="cpu", tracker_factory=score._StartTracker, mode="map", map_factory=factory,
                    map_renderer=base._Renderer(), map_config=MapConfig(**cfg))
    loc.reset(*score._frame_at(torch.eye(4)), torch.eye(4))
    score._ScoreMirrorMap.log = []
    return loc


ALIGN_FIELDS = ("aligned", "align_status", "align_steps", "align_from", "align_moved_t", "align_moved_r_deg",
                "align_scores")
MOVED = score._shift(2, -0.02)  # back along the optical axis: every depth grows by 2 cm


def test_align_pose_of_a_map_on_the_mirror():
    m = _AlignMirrorMap(W, H, MapConfig(align=True), "cpu")
    K = replica_intrinsics(W, H)
    depth, rgb = score._frame_at(torch.eye(4))
    score._ScoreMirrorMap.log = []
    empty = m.align_pose(depth, K, torch.eye(4), CFG_NEAR)
    assert isinstance(empty, PoseAlignment) and (empty.status, empty.steps, empty.used, empty.moved) == ("FEW", 0, 0, False)
    assert score._ScoreMirrorMap.log == [] and torch.equal(empty.c2w, torch.eye(4))
    m.insert_frame(depth, rgb, K, torch.eye(4))
    query, _ = score._frame_at(MOVED, 1)
    al = m.align_pose(query, K, torch.eye(4), CFG_NEAR)
    call = score._ScoreMirrorMap.log[-1]
    assert call["call"] == "align" and call["rows"] == W * H and call["near"] == CFG_NEAR and call["steps"] == 8
    assert (call["keep"], call["beyond"], call["kappa"]) == (float(KEEP), float(BEYOND), float(KAPPA))
    assert (call["damping"], call["min_used"]) == (1e-3, 7) and np.array_equal(call["w2c"], np.eye(4, dtype=F32))
    assert call["bounds"] == (math.radians(12.8), 0.32) and call["eps"] == (math.radians(1.5e-4), 3e-5)
    assert al.status in mapping.ALIGN_STATUS and al.steps == call["taken"] and len(al.history) == 8
    assert al.w2c64.dtype == np.float64 and same_bits(al.w2c64[:3], call["pose"]) and al.w2c64[3].tolist() == [0, 0, 0, 1]
    assert al.c2w.dtype == torch.float32 and al.c2w.shape == (4, 4)
    assert same_bits(al.c2w.numpy(), np.linalg.inv(al.w2c64).astype(F32))  # inverted in float64, rounded once
    assert [h[0] for h in al.history] == [ref.NAMES[s] for s in call["history"][:, 0]]
    assert (al.used, al.tested) == (int(call["history"][-1, 1]), int(call["history"][-1, 2])) and al.history[0][4].shape == (6,)
    # the arguments of the call win over the configuration's
    m.align_pose(query, K, torch.eye(4), CFG_NEAR, steps=3, rho=0.25, kappa=0.5, damping=0.0, max_rot_deg=1.0,
                 max_trans=0.5, eps_rot_deg=0.0, eps_trans=0.0, min_used=9)
    call = score._ScoreMirrorMap.log[-1]
    assert (call["steps"], call["keep"], call["beyond"], call["kappa"], call["damping"], call["min_used"]) == (
        3, 0.75, 1.25, 0.5, 0.0, 9)
    assert call["bounds"] == (math.radians(1.0), 0.5) and call["eps"] == (0.0, 0.0)
    m2 = _AlignMirrorMap(W, H, MapConfig(align_rho=0.125, depth_rho=0.05, info_kappa=0.25, align_steps=2,
                                         align_damping=0.5), "cpu")
    m2.insert_frame(depth, rgb, K, torch.eye(4))
    assert len(m2.align_pose(query, K, torch.eye(4), CFG_NEAR).history) == 2
    call = score._ScoreMirrorMap.log[-1]
    assert (call["keep"], call["beyond"], call["kappa"], call["damping"]) == (0.875, 1.125, 0.25, 0.5)
    for bad in (dict(steps=0), dict(steps=33), dict(rho=1.0), dict(kappa=-1.0), dict(damping=float("nan")),
                dict(max_trans=0.0), dict(eps_trans=-1.0), dict(min_used=6)):
        with pytest.raises(ValueError, match=list(bad)[0].split("_")[0]):
            m.align_pose(query, K, torch.eye(4), CFG_NEAR, **bad)
    with pytest.raises(ValueError, match=r"\(4, 4\)"):
        m.align_pose(query, K, torch.eye(3), CFG_NEAR)
    host = mapping.GaussianMap(W, H, MapConfig(), "cpu")
    host.n_live = 3
    with pytest.raises(AssertionError, match="no CPU path"):
        host.align_pose(query, K, torch.eye(4), CFG_NEAR)


def test_without_the_option_the_alignment_is_never_asked(monkeypatch):
    def never(*a, **k):
        raise AssertionError("align_pose without MapConfig.align")

    monkeypatch.setattr(mapping.GaussianMap, "align_pose", never)
    loc = _localizer(monkeypatch)
    r = loc.track(*score._frame_at(MOVED, 1))
    assert [c["call"] for c in score._ScoreMirrorMap.log] == ["insert"] and loc.map._align is None
    assert all(getattr(r, f) is None for f in ALIGN_FIELDS) and not r.lost
    assert torch.equal(r.init_c2w, torch.eye(4)) and torch.equal(score._StartTracker.made[0].loads[0]["tar_c2w"], torch.eye(4))
    assert all(getattr(LocalizeResult(torch.eye(4), torch.eye(4), 1, 1, 0.0, False), f) is None for f in ALIGN_FIELDS)


def test_with_the_option_the_tracker_starts_from_the_aligned_pose(monkeypatch, capsys):
    loc = _localizer(monkeypatch, align=True)
    depth, rgb = score._frame_at(MOVED, 1)
    r = loc.track(depth, rgb, gt_c2w=MOVED)
    assert [c["call"] for c in score._ScoreMirrorMap.log] == ["align", "score", "insert"]
    call, scored = score._ScoreMirrorMap.log[:2]
    assert np.array_equal(call["w2c"], np.eye(4, dtype=F32)) and torch.equal(call["depth"], depth) and call["rows"] == W * H
    w2c64 = np.vstack([call["pose"], [0.0, 0.0, 0.0, 1.0]])
    want = torch.from_numpy(np.linalg.inv(w2c64).astype(F32))
    assert call["taken"] >= 1 and scored["w2c"].shape == (2, 4, 4)
    assert np.array_equal(scored["w2c"][0], np.eye(4, dtype=F32)) and np.array_equal(scored["w2c"][1], info.w2c_of(want.numpy()))
    margin = scored["counts"][:, 1] - scored["counts"][:, 2]
    with capsys.disabled():
        print(f"[align] stand-in frame 2 cm back: {r.align_status} after {r.align_steps} steps, moved {r.align_moved_t:.3e} m "
              f"{r.align_moved_r_deg:.3e} deg, start eT {float(torch.norm(want[:3, 3] - MOVED[:3, 3])):.3e}, margins "
              f"{margin.tolist()}")
    assert margin[1] >= margin[0] and r.align_scores == tuple(tuple(c) for c in scored["counts"].tolist())
    assert r.aligned is True and r.align_status in ("CONVERGED", "STEPPED") and r.align_steps == call["taken"]
    assert torch.equal(r.align_from, torch.eye(4)) and torch.equal(r.init_c2w, want)
    assert r.align_moved_t == float(torch.norm(want[:3, 3])) > 0.0 and r.align_moved_r_deg >= 0.0
    assert float(torch.norm(want[:3, 3] - MOVED[:3, 3])) < 0.02  # nearer to the frame's pose than the start was
    loads = [load for t in score._StartTracker.made for load in t.loads]
    assert len(loads) == 1 and torch.equal(loads[0]["tar_c2w"], want) and torch.equal(r.c2w, want)
    assert torch.equal(score._ScoreMirrorMap.log[2]["c2w"], want) and not r.lost and r.steps == 12


def test_an_alignment_that_scores_worse_is_dropped(monkeypatch):
    loc = _localizer(monkeypatch, factory=_WorseMap, align=True)
    r = loc.track(*score._frame_at(MOVED, 1))
    assert [c["call"] for c in score._ScoreMirrorMap.log] == ["align", "score", "insert"]
    assert r.aligned is False and r.align_status in ("CONVERGED", "STEPPED") and r.align_steps >= 1 and r.align_moved_t > 0.0
    assert torch.equal(r.init_c2w, torch.eye(4)) and torch.equal(r.align_from, torch.eye(4))
    loads = [load for t in score._StartTracker.made for load in t.loads]
    assert len(loads) == 1 and torch.equal(loads[0]["tar_c2w"], torch.eye(4)) and torch.equal(r.c2w, torch.eye(4))


def test_rows_that_leave_the_view_do_not_count_against_the_alignment(monkeypatch):
    """The share of the rows judged that agree decides, not agree - front: a camera that moves loses rows over the
    image's edge, and a pose that follows it must not lose to the one that stayed behind for that."""
    loc = _localizer(monkeypatch, factory=_FewerRowsMap, align=True)
    r = loc.track(*score._frame_at(MOVED, 1))
    (t0, a0, f0), (t1, a1, f1) = r.align_scores
    assert (t1, a1, f1) == (t0 - 10, a0 - 10, f0) and a1 - f1 < a0 - f0 and a1 * f0 >= a0 * f1
    assert r.aligned is True and not torch.equal(r.init_c2w, torch.eye(4))


def test_an_alignment_with_too_few_rows_is_dropped_without_a_score(monkeypatch):
    loc = _localizer(monkeypatch, align=True)
    depth, rgb = score._frame_at(MOVED, 1)
    r = loc.track(depth * 1.5, rgb)  # no row of the map agrees with a frame half as far again
    assert [c["call"] for c in score._ScoreMirrorMap.log] == ["align", "insert"]
    assert (score._ScoreMirrorMap.log[0]["history"][:, 0] == ref.FEW).all()
    assert (r.aligned, r.align_status, r.align_steps, r.align_moved_t, r.align_moved_r_deg, r.align_scores) == (
        False, "FEW", 0, 0.0, 0.0, None)
    assert torch.equal(r.init_c2w, torch.eye(4)) and torch.equal(score._StartTracker.made[0].loads[0]["tar_c2w"], torch.eye(4))


def test_the_aligned_start_is_what_the_relocalisation_sees(monkeypatch):
    """reloc with the option: the estimate is scored after the alignment's own score call, and the flow is the one
    without the option from the aligned start on."""
    loc = _localizer(monkeypatch, align=True, reloc=True)
    r = loc.track(*score._frame_at(MOVED, 1), gt_c2w=MOVED)
    assert [(c["call"], len(c.get("w2c", []))) for c in score._ScoreMirrorMap.log] == [
        ("align", 4), ("score", 2), ("score", 1), ("insert", 0)]
    assert r.aligned and not r.lost and r.relocalised is False and torch.equal(r.init_c2w, r.c2w)


def test_the_option_of_the_evaluation_driver_needs_the_map_mode(tmp_path, capsys):
    from gsplatloc_amd import eval as ev

    with pytest.raises(ValueError, match="map_align"):
        ev.evaluate_room(None, 200, 3, sequential=True, map_align=True)
    with pytest.raises(ValueError, match="map_align_steps"):
        ev.evaluate_room(None, 200, 3, sequential=True, map_mode=True, map_align_steps=4)
    for extra, why in ((["--map-align"], "needs --map"), (["--sequential", "--map-align"], "needs --map"),
                       (["--sequential", "--map", "--map-align-steps", "4"], "needs --map-align")):
        with pytest.raises(SystemExit):
            ev.main(["--root", str(tmp_path)] + extra)
        assert why in capsys.readouterr().err
