"""Pose information (csrc/map_info.hip, GaussianMap.pose_information, MapConfig.info), the parts that need no GPU: the
numpy mirror tests/map_info_ref.py (float32 and fixed point, as the kernel) on a view into a corner, where the
Gauss-Newton step must give a known twist back, and on one plane, where three of the six directions are open; the
host's PoseInformation and apply_twist; MapConfig; the entry point against its prototype and its argument checks; the
kernel's budget; and Localizer(mode="map") with ``info`` around the stand-ins of tests/test_map_score_cpu.py and a map
whose device calls are the mirrors.

The corner view (160x120, gsplatloc_amd.synthetic.room_depth): the map is the back-projection of one frame at position
(0.6, 0.1, 0.8), yaw 35 degrees about y; the query frame is taken 5 cm and 4 cm from there at yaw 38; the estimate is
the query's true pose perturbed by a twist xi = (omega, upsilon), w2c_est = exp(xi^) w2c_true.  Three twists from one
default_rng(0): normal(size=3) * 0.2 degrees / 1.7 for omega, then normal(size=3) * 3 mm / 1.7 for upsilon, per twist.
The float64 prototype of this set-up gave delta = -H^-1 g within 0.1 % of -omega and 2.1 % of -upsilon with the
planarity test at kappa = 1e-3, and 30 .. 90 % off in the y translation without it (the rows at the room's creases).
The bound here is 10 % of |omega| and of |upsilon|: five times that worst figure, which leaves room for float32 and the
2^-20 fixed point, and an order of magnitude below the failure without the test.  What the mirror measures is printed
(NOTES.md, "Pose information")."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from gsplatloc_amd import _lib, mapping
from gsplatloc_amd.localizer import Localizer, LocalizeResult
from gsplatloc_amd.mapping import GaussianMap, MapConfig, PoseInformation, apply_twist
from gsplatloc_amd.my_gsplat import TrackerConfig
from gsplatloc_amd.synthetic import replica_intrinsics, room_depth
from tests import map_info_ref as ref
from tests import test_map_cpu as base
from tests import test_map_score_cpu as score
from tests.test_abi import prototypes
from tests.test_kernel_resources import HIPCC, _resources

F32 = np.float32
NEAR = 0.01
KAPPA = 1e-3


def intrinsics(K):
    return tuple(float(a) for a in (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))


def yaw_pose(position, yaw_deg):
    """float64 [4,4] camera to world: the camera at ``position``, turned by yaw_deg about y."""
    c, s = math.cos(math.radians(yaw_deg)), math.sin(math.radians(yaw_deg))
    T = np.eye(4)
    T[:3, :3] = [[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]
    T[:3, 3] = position
    return T


def back_projection(depth, intr, c2w):
    """float32 [h*w,3] in the world, with k_map_append's expression: ((u - cx) / fx * d, (v - cy) / fy * d, d), R p + t."""
    d = np.asarray(depth, F32)
    v, u = np.mgrid[0:d.shape[0], 0:d.shape[1]]
    fx, fy, cx, cy = (F32(a) for a in intr)
    p = np.stack([(u.astype(F32) - cx) / fx * d, (v.astype(F32) - cy) / fy * d, d], -1).reshape(-1, 3)
    c = np.asarray(c2w, F32)
    return np.stack([((c[j, 0] * p[:, 0] + c[j, 1] * p[:, 1]) + c[j, 2] * p[:, 2]) + c[j, 3] for j in range(3)], 1)


def information(out, min_eig=mapping.INFO_MIN_EIG):
    return PoseInformation(*ref.unpack(out), min_eig)


# ---- (a) the corner view: the step gives the twist back -------------------------------------------------------------
CW, CH = 160, 120


@pytest.fixture(scope="module")
def corner():
    K = replica_intrinsics(CW, CH)
    intr = intrinsics(K)
    at_map, at_query = yaw_pose((0.6, 0.1, 0.8), 35.0), yaw_pose((0.65, 0.1, 0.76), 38.0)
    d_map = room_depth(CW, CH, K, torch.from_numpy(at_map).float()).numpy()
    d_query = room_depth(CW, CH, K, torch.from_numpy(at_query).float()).numpy()
    rng = np.random.default_rng(0)
    twists = [np.concatenate([rng.normal(size=3) * math.radians(0.2) / 1.7, rng.normal(size=3) * 0.003 / 1.7])
              for _ in range(3)]
    return dict(intr=intr, means=back_projection(d_map, intr, at_map), depth=d_query, truth=at_query, twists=twists)


def _sums(c, xi, kappa):
    est = apply_twist(torch.from_numpy(c["truth"]), xi).numpy()  # w2c_est = exp(xi^) w2c_true
    return ref.pose_info(c["means"], ref.w2c_of(est), c["intr"], c["depth"], ref.keep_of(0.05), ref.beyond_of(0.05),
                         kappa, NEAR)


def test_the_step_gives_the_twist_back_in_a_corner(corner, capsys):
    for i, xi in enumerate(corner["twists"]):
        info = information(_sums(corner, xi, KAPPA))
        delta, cov = info.step(), info.covariance()
        assert not info.weak() and delta is not None and cov is not None
        rot = float(np.linalg.norm(delta[:3] + xi[:3]) / np.linalg.norm(xi[:3]))
        trans = float(np.linalg.norm(delta[3:] + xi[3:]) / np.linalg.norm(xi[3:]))
        with capsys.disabled():
            print(f"[info] corner twist {i}: used {info.used} of {CW * CH} (tested {info.tested}), |d_rot + omega| / "
                  f"|omega| {rot:.3e}, |d_trans + upsilon| / |upsilon| {trans:.3e}, eigenvalues of H / used "
                  f"{info.eigenvalues[0]:.3e} .. {info.eigenvalues[-1]:.3e}")
        assert rot <= 0.1 and trans <= 0.1, (i, rot, trans)
        assert 16000 < info.used <= info.tested < CW * CH
        assert np.array_equal(cov, cov.T) or np.allclose(cov, cov.T, rtol=1e-9, atol=0.0)
        assert np.all(np.linalg.eigvalsh(cov) > 0.0)
        # the step is the pose's: applied to the estimate it lands on the truth
        est = apply_twist(torch.from_numpy(corner["truth"]), xi)
        back = apply_twist(est, delta).numpy()
        assert np.linalg.norm(back[:3, 3] - corner["truth"][:3, 3]) <= 0.1 * np.linalg.norm(xi[3:]) + 1e-4


def test_without_the_planarity_test_the_creases_bias_the_step(corner):
    """The reason for kappa: with the test switched off (a kappa no patch fails) the rows at the creases come in and the
    translation is off by more than the bound of the test above, for every twist."""
    for xi in corner["twists"]:
        with_test, without = information(_sums(corner, xi, KAPPA)), information(_sums(corner, xi, 1e9))
        assert without.used == without.tested > with_test.used
        delta = without.step()
        assert np.linalg.norm(delta[3:] + xi[3:]) > 0.1 * np.linalg.norm(xi[3:])


# ---- (b) one plane --------------------------------------------------------------------------------------------------
PW, PH, PINTR = 33, 17, (32.0, 32.0, 16.0, 8.0)
PK = torch.tensor([[PINTR[0], 0.0, PINTR[2]], [0.0, PINTR[1], PINTR[3]], [0.0, 0.0, 1.0]])


def plane_case():
    depth = np.full((PH, PW), 2.0, F32)
    return depth, back_projection(depth, PINTR, np.eye(4))


def test_one_plane_leaves_three_directions_open():
    depth, means = plane_case()
    out = ref.pose_info(means, np.eye(4, dtype=F32), PINTR, depth, ref.keep_of(0.05), ref.beyond_of(0.05), KAPPA, NEAR)
    inner = (PW - 2) * (PH - 2)
    assert out[28] == out[29] == inner and out.dtype == np.int64
    # n = (0, 0, +-1) exactly: every product with J's entries omega_z, upsilon_x, upsilon_y is an exact zero
    for slot, (a, b) in enumerate(ref.SLOTS):
        if {a, b} & {2, 3, 4}:
            assert out[slot] == 0, (slot, a, b)
    assert out[ref.SLOTS.index((5, 5))] == inner << 20  # n_z^2 = 1 per row
    assert out[27] == 0 and not out[21:27].any()  # the rows lie on the plane: r == 0
    info = information(out)
    assert info.eigenvalues[0] == 0.0 and info.eigenvalues[3] > 0.0  # three open, three held
    assert info.weak() and info.step() is None and info.covariance() is None


def test_pose_information_of_a_map_on_the_mirror():
    depth, means = plane_case()
    m = _InfoMirrorMap(PW, PH, MapConfig(info=True), "cpu")
    score._ScoreMirrorMap.log = []
    empty = m.pose_information(depth, PK, torch.eye(4), NEAR)
    assert (empty.used, empty.tested, empty.weak(), empty.step()) == (0, 0, True, None) and score._ScoreMirrorMap.log == []
    rgb = torch.zeros(PH, PW, 3)
    assert m.insert_frame(torch.from_numpy(depth), rgb, PK, torch.eye(4)) == (PW * PH, PW * PH)
    assert np.array_equal(m.points.numpy(), means)
    info = m.pose_information(depth, PK, torch.eye(4), NEAR)
    call = score._ScoreMirrorMap.log[-1]
    assert call["call"] == "info" and call["rows"] == PW * PH and call["near"] == NEAR
    assert (call["keep"], call["beyond"]) == (float(ref.keep_of(0.05)), float(ref.beyond_of(0.05)))
    assert call["kappa"] == float(F32(1e-3)) and np.array_equal(call["w2c"], np.eye(4, dtype=F32))
    assert info.used == info.tested == (PW - 2) * (PH - 2) and info.weak() and info.covariance() is None
    assert info.H.dtype == np.float64 and info.H.shape == (6, 6) and info.g.shape == (6,) and np.array_equal(info.H, info.H.T)
    assert info.H[5, 5] == float(info.used) and not info.H[2:5].any()
    # rho and kappa of the call win over the configuration's; info_rho over depth_rho
    m.pose_information(depth, PK, torch.eye(4), NEAR, rho=0.25, kappa=0.5)
    call = score._ScoreMirrorMap.log[-1]
    assert (call["keep"], call["beyond"], call["kappa"]) == (0.75, 1.25, 0.5)
    m2 = _InfoMirrorMap(PW, PH, MapConfig(info_rho=0.125, depth_rho=0.05, info_kappa=0.25, info_min_eig=0.5), "cpu")
    m2.insert_frame(torch.from_numpy(depth), rgb, PK, torch.eye(4))
    assert m2.pose_information(depth, PK, torch.eye(4), NEAR).min_eig == 0.5
    call = score._ScoreMirrorMap.log[-1]
    assert (call["keep"], call["beyond"], call["kappa"]) == (0.875, 1.125, 0.25)
    for bad in (dict(rho=1.0), dict(rho=-0.1), dict(kappa=-1.0), dict(kappa=float("nan"))):
        with pytest.raises(ValueError, match=list(bad)[0]):
            m.pose_information(depth, PK, torch.eye(4), NEAR, **bad)
    with pytest.raises(ValueError, match="depth"):
        m.pose_information(np.ones((PH, PW + 1), F32), PK, torch.eye(4), NEAR)
    with pytest.raises(ValueError, match=r"\(4, 4\)"):
        m.pose_information(depth, PK, torch.eye(3), NEAR)
    host = GaussianMap(PW, PH, MapConfig(), "cpu")
    host.n_live = 3
    with pytest.raises(AssertionError, match="no CPU path"):
        host.pose_information(depth, PK, torch.eye(4), NEAR)


# ---- PoseInformation and apply_twist --------------------------------------------------------------------------------
def test_pose_information_on_hand_made_sums():
    H = np.diag([4.0, 9.0, 16.0, 25.0, 36.0, 49.0])
    g = np.array([4.0, -9.0, 16.0, 0.0, 36.0, -49.0])
    info = PoseInformation(H, g, rss=8.0, used=10, tested=12)
    assert np.allclose(info.eigenvalues, np.array([0.4, 0.9, 1.6, 2.5, 3.6, 4.9])) and info.min_eig == mapping.INFO_MIN_EIG
    assert not info.weak() and info.weak(0.41) and not info.weak(0.4)
    assert np.allclose(info.step(), [-1.0, 1.0, -1.0, 0.0, -1.0, 1.0])
    assert np.allclose(info.covariance(), 2.0 * np.diag(1.0 / np.diag(H)))  # sigma^2 = 8 / (10 - 6)
    few = PoseInformation(H, g, rss=8.0, used=6, tested=12)
    assert few.weak() and few.step() is None and few.covariance() is None
    assert not PoseInformation(H, g, rss=8.0, used=7, tested=12).weak()
    flat = PoseInformation(np.diag([4.0, 9.0, 0.0, 25.0, 36.0, 49.0]), g, 8.0, 10, 12)
    assert flat.weak() and flat.step() is None and flat.covariance() is None


def test_apply_twist_is_the_left_perturbation_of_the_world_to_camera_pose():
    c2w = torch.from_numpy(yaw_pose((0.3, -0.2, 1.1), 25.0))
    xi = np.array([0.02, -0.03, 0.01, 0.05, -0.04, 0.02])
    moved = apply_twist(c2w, xi)
    assert moved.dtype == torch.float64 and moved.shape == (4, 4)
    rel = np.linalg.inv(moved.numpy()) @ c2w.numpy()  # w2c' c2w = exp(xi^)
    assert np.allclose(rel[3], [0, 0, 0, 1]) and np.allclose(rel[:3, :3] @ rel[:3, :3].T, np.eye(3), atol=1e-12)
    p = np.array([0.4, -0.7, 2.0])
    first_order = p + np.cross(xi[:3], p) + xi[3:]
    assert np.linalg.norm(rel[:3, :3] @ p + rel[:3, 3] - first_order) < 3e-3  # second order in |xi| = 0.08
    tiny = 1e-7 * xi
    rel = np.linalg.inv(apply_twist(c2w, tiny).numpy()) @ c2w.numpy()
    assert np.allclose(rel[:3, :3] @ p + rel[:3, 3], p + np.cross(tiny[:3], p) + tiny[3:], atol=1e-13)
    assert torch.equal(apply_twist(c2w, np.zeros(6)), c2w)
    assert torch.allclose(apply_twist(apply_twist(c2w, xi), -xi), c2w, atol=1e-12)
    assert apply_twist(c2w.float(), xi).dtype == torch.float32
    with pytest.raises(ValueError, match=r"\(4, 4\)"):
        apply_twist(torch.eye(3), xi)


# ---- MapConfig ------------------------------------------------------------------------------------------------------
def test_map_config_validation():
    c = MapConfig()
    assert (c.info, c.info_rho, c.info_kappa, c.info_min_eig) == (False, None, 1e-3, None)
    ok = MapConfig(info=True, info_rho=0.0, info_kappa=0.0, info_min_eig=1e-6)
    assert ok.info and MapConfig(info=True, depth_rho=0.0).info
    bad = dict(info=[1, "yes", None, 0.5],
               info_rho=[1.0, -0.01, float("nan"), True, "0.05"],
               info_kappa=[-1e-3, float("inf"), float("nan"), True, None, "1e-3"],
               info_min_eig=[0.0, -1.0, float("inf"), float("nan"), True, "1e-3"])
    for field, values in bad.items():
        for v in values:
            with pytest.raises(ValueError, match=field):
                MapConfig(**{field: v})
    for rho in (1.0, -0.01, 1.5):
        with pytest.raises(ValueError, match="depth_rho"):
            MapConfig(info=True, depth_rho=rho)
        assert MapConfig(info=True, depth_rho=rho, info_rho=0.05).info  # its own fraction is what it needs
        assert MapConfig(depth_rho=rho).depth_rho == rho  # only the option needs it


# ---- the entry point ------------------------------------------------------------------------------------------------
BAD_ARG = -1
FN = "gsl_map_pose_info"
GOOD = dict(n_rows=1000, fx=50.0, fy=40.0, cx=31.5, cy=23.5, width=64, height=48, keep=0.95, beyond=1.05, kappa=1e-3,
            near_plane=0.01)
GOOD_MAX_ROWS = ref.max_rows((50.0, 40.0, 31.5, 23.5), 64, 48, 0.95)
REFUSED = [
    ("NULL means", dict(means=None)), ("NULL w2c", dict(w2c=None)), ("NULL depth", dict(depth=None)),
    ("NULL out", dict(out=None)), ("n_rows == 0", dict(n_rows=0)), ("n_rows < 0", dict(n_rows=-5)),
    ("n_rows == 2^31", dict(n_rows=1 << 31)), ("n_rows beyond 2^32", dict(n_rows=(1 << 32) + 7)),
    ("a sum could overflow", dict(n_rows=GOOD_MAX_ROWS + 1)),
    ("a wide angle: fewer rows", dict(n_rows=1000, fx=1e-3, fy=1e-3)),
    ("a principal point far away: fewer rows", dict(n_rows=1000, cx=1e9)),
    ("a NaN principal point", dict(cy=float("nan"))),
    ("width <= 0", dict(width=0)), ("height <= 0", dict(height=-3)), ("2^31 pixels", dict(width=65536, height=32768)),
    ("fx == 0", dict(fx=0.0)), ("fy == 0", dict(fy=0.0)), ("fx == -0", dict(fx=-0.0)),
    ("keep == 0", dict(keep=0.0)), ("keep < 0", dict(keep=-0.5)), ("keep > 1", dict(keep=1.0000001)),
    ("NaN keep", dict(keep=float("nan"))), ("beyond < 1", dict(beyond=0.9999999)), ("beyond < 0", dict(beyond=-2.0)),
    ("NaN beyond", dict(beyond=float("nan"))), ("inf beyond", dict(beyond=float("inf"))),
    ("kappa < 0", dict(kappa=-1e-3)), ("NaN kappa", dict(kappa=float("nan"))), ("inf kappa", dict(kappa=float("inf"))),
]


def call_with(lib, params, named, pointers):
    """gsl_map_pose_info with the named arguments over GOOD; ``pointers``: parameter name -> address."""
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
    assert ret == "int" and [n for _, n in params] == [
        "means", "n_rows", "w2c", "fx", "fy", "cx", "cy", "depth", "width", "height", "keep", "beyond", "kappa",
        "near_plane", "out", "stream"]
    assert dict((n, t) for t, n in params)["out"] == "int64_t*"
    assert len(_lib._SIGNATURES[FN][1]) == len(params)
    src = open(os.path.join(repo_root, "gsplatloc_amd", "csrc", "map_info.hip")).read()
    m = re.search(r'extern "C" int gsl_map_pose_info\((.*?)\)\s*\{', src, flags=re.S)
    assert m, "no definition of gsl_map_pose_info"
    defined = [re.fullmatch(r"\s*(.*?)\s*(\w+)\s*", p, flags=re.S).groups() for p in m.group(1).split(",")]
    assert [(" ".join(t.split()), n) for t, n in defined] == params
    header = open(os.path.join(repo_root, "include", "gsloc_hip.h")).read()
    values = int(re.search(r"#define GSL_MAP_INFO_VALUES (\d+)", header).group(1))
    assert values == 30 == mapping.INFO_VALUES == ref.VALUES == _lib.load_library().gsl_map_info_values()
    assert "map_info.hip" in open(os.path.join(repo_root, "gsplatloc_amd", "csrc", "Makefile")).read()
    assert "#pragma clang fp contract(off)" in src and "atomicAdd(float" not in src
    # the row projection is the one copy of map_dev.h
    assert "map_project_point(" in src and not re.search(r"w2c\[\d+\]\s*\*", src)


def test_the_row_bound_is_the_mirrors():
    lib = _lib.load_library()
    cases = [((50.0, 40.0, 31.5, 23.5), 64, 48, 0.95), ((80.0, 105.88235, 79.5, 59.5), 160, 120, 0.95),
             ((600.0, 600.0, 599.5, 339.5), 1200, 680, 0.5), ((1.0, 1.0, 100.0, 100.0), 200, 200, 0.01),
             ((1e-3, 1e-3, 0.0, 0.0), 3, 3, 1.0), ((-50.0, 40.0, 31.5, 23.5), 64, 48, 1.0)]
    for intr, w, h, keep in cases:
        got, want = lib.gsl_map_info_max_rows(*intr, w, h, keep), ref.max_rows(intr, w, h, keep)
        assert abs(got - want) <= max(1, want >> 40) and 0 < got <= 2 ** 31 - 1, (intr, got, want)
    assert lib.gsl_map_info_max_rows(*cases[1][0], 160, 120, 0.95) > 10 ** 8  # a tracked frame's map is far inside
    # B bounds every entry of J and r: with it no sum of n terms leaves 63 bits
    intr, w, h, keep = cases[1]
    tx, ty = (w - 1.5 - intr[2]) / intr[0], (h - 1.5 - intr[3]) / intr[1]
    B = 64.0 * math.sqrt(1.0 + tx * tx + ty * ty) * (1.0 + 1.0 / keep)
    assert ref.max_rows(intr, w, h, keep) * (B * B * 2.0 ** 20 + 1.0) < 2.0 ** 63
    for bad in ((0.0, 40.0, 31.5, 23.5, 64, 48, 0.95), (50.0, 40.0, 31.5, 23.5, 0, 48, 0.95),
                (50.0, 40.0, 31.5, 23.5, 64, 48, 0.0), (50.0, 40.0, float("nan"), 23.5, 64, 48, 0.95)):
        assert lib.gsl_map_info_max_rows(*bad) == 0


def test_entry_point_rejects_bad_arguments_before_any_launch(repo_root):
    """Every row is refused on the host: the pointers are one dummy HOST buffer, a launch (the zeroing of out is one)
    would give GSL_ERR_HIP or worse."""
    lib = _lib.load_library()
    params = prototypes(repo_root)[FN][1]
    buf = ctypes.create_string_buffer(b"\x7f" * 1024, 1024)
    pointers = {n: ctypes.addressof(buf) for t, n in params if "*" in t}
    for what, over in REFUSED:
        named = dict(GOOD, **over)
        assert set(named) <= {n for _, n in params}, what
        assert call_with(lib, params, named, pointers) == BAD_ARG, what
    assert buf.raw == b"\x7f" * 1024  # nothing wrote to the buffer


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_the_info_kernel_stays_in_registers():
    """k_map_pose_info: 28 64-bit sums per lane and no scratch, no accumulation registers, the table of 30 sums in LDS,
    at least four waves per SIMD (the grid cap is four workgroups per CU)."""
    hit = [v for k, v in _resources("map_info.hip").items() if "k_map_pose_info" in k]
    assert len(hit) == 1
    r = hit[0]
    assert r["ScratchSize"] == 0 and r["AGPRs"] == 0 and r["LDS"] == 30 * 8 and r["VGPRs"] <= 128, r
    assert r["Occupancy"] >= 4, r


# ---- Localizer(mode="map", info) around the mirrors ----------------------------------------------------------------
W, H = base.W, base.H
CFG_NEAR = TrackerConfig().gs.near_plane


class _InfoMirrorMap(score._ScoreMirrorMap):
    """The stand-in map of tests/test_map_score_cpu.py with the mirror of csrc/map_info.hip; one log for all calls."""

    def _info_launch(self, depth, intr, w2c, keep, beyond, kappa, near):
        sums = ref.pose_info(self.means[:self.n_live].numpy(), w2c.numpy(), intr, depth.numpy(), F32(keep), F32(beyond),
                             F32(kappa), near)
        score._ScoreMirrorMap.log.append(dict(call="info", w2c=w2c.numpy().copy(), depth=depth.clone(), near=near,
                                              rows=self.n_live, keep=keep, beyond=beyond, kappa=kappa, sums=sums))
        return sums


def _localizer(tracker, monkeypatch, **cfg):
    import gsplatloc_amd.data.dataset as DS

    monkeypatch.setattr(DS, "compute_depth_gt", lambda pts, col, Ks, c2w, height, width: torch.zeros(height, width))
    tracker.made = base._Tracker.made = []
    loc = Localizer(replica_intrinsics(W, H), W, H, TrackerConfig(max_steps=5), normalize=False, motion="hold",
                    device="cpu", tracker_factory=tracker, mode="map", map_factory=_InfoMirrorMap,
                    map_renderer=base._Renderer(), map_config=MapConfig(**cfg))
    loc.reset(*score._frame_at(torch.eye(4)), torch.eye(4))
    score._ScoreMirrorMap.log = []
    return loc


INFO_FIELDS = ("cov", "sigma_t", "sigma_r", "info_used", "info_min_eig", "weak")


def test_without_the_option_nothing_is_asked(monkeypatch):
    loc = _localizer(score._StartTracker, monkeypatch)
    r = loc.track(*score._frame_at(torch.eye(4), 1))
    assert [c["call"] for c in score._ScoreMirrorMap.log] == ["insert"] and loc.map._info is None
    assert all(getattr(r, f) is None for f in INFO_FIELDS) and not r.lost
    assert all(getattr(LocalizeResult(torch.eye(4), torch.eye(4), 1, 1, 0.0, False), f) is None for f in INFO_FIELDS)


def test_with_the_option_one_call_per_frame_before_the_map_is_touched(monkeypatch):
    plain = _localizer(score._StartTracker, monkeypatch)
    frames = [score._frame_at(torch.eye(4), 1), score._frame_at(score._shift(0, 0.02), 2)]
    want = [plain.track(*f) for f in frames]
    want_points = plain.map.points.clone()
    loc = _localizer(score._StartTracker, monkeypatch, info=True)
    for i, (depth, rgb) in enumerate(frames):
        score._ScoreMirrorMap.log = []
        rows_before = loc.map.n_live
        r = loc.track(depth, rgb)
        assert [c["call"] for c in score._ScoreMirrorMap.log] == ["info", "insert"]
        call = score._ScoreMirrorMap.log[0]
        assert call["rows"] == rows_before and call["near"] == CFG_NEAR and torch.equal(call["depth"], depth)
        assert np.array_equal(call["w2c"], ref.w2c_of(r.c2w.numpy()))  # at the frame's final estimate
        assert (call["keep"], call["beyond"], call["kappa"]) == (
            float(ref.keep_of(0.05)), float(ref.beyond_of(0.05)), float(F32(1e-3)))
        info = information(call["sums"])
        assert r.info_used == info.used > 0 and r.weak == info.weak() and r.info_min_eig == float(info.eigenvalues[0])
        if r.weak:
            assert r.cov is None and r.sigma_t is None and r.sigma_r is None
        else:
            assert np.array_equal(r.cov, info.covariance())
            assert r.sigma_t == math.sqrt(np.trace(r.cov[3:, 3:]))
            assert r.sigma_r == math.degrees(math.sqrt(np.trace(r.cov[:3, :3])))
        # nothing is gated on it: the frame is what it is without the option
        assert (r.steps, r.best_step, r.added, r.map_size, r.lost) == (
            want[i].steps, want[i].best_step, want[i].added, want[i].map_size, want[i].lost)
        assert torch.equal(r.c2w, want[i].c2w)
    assert torch.equal(loc.map.points, want_points)


def test_the_call_follows_the_relocalisation_and_a_lost_frame_is_not_asked(monkeypatch):
    loc = _localizer(score._StartTracker, monkeypatch, info=True, reloc=True, reloc_trans=score.STEP, reloc_rot_deg=3.0)
    truth = score._shift(2, -score.STEP)
    r = loc.track(*score._frame_at(truth, 1), gt_c2w=truth)
    # the start is rejected, the grid's winner tracked and accepted: only then, at that estimate, the one call
    assert [c["call"] for c in score._ScoreMirrorMap.log] == ["score", "score", "score", "info", "insert"]
    assert r.relocalised and not r.lost and r.weak is not None and r.info_used > 0
    assert np.array_equal(score._ScoreMirrorMap.log[3]["w2c"], ref.w2c_of(truth.numpy()))
    lost = _localizer(score._StartTrackerWithoutMinimum, monkeypatch, info=True, reloc=True)
    r = lost.track(*score._frame_at(torch.eye(4), 1))
    assert r.lost and [c["call"] for c in score._ScoreMirrorMap.log] == ["score", "score"]
    assert all(getattr(r, f) is None for f in INFO_FIELDS)
    gone = _localizer(base._LostTracker, monkeypatch, info=True)  # no reloc: lost is "no minimum was recorded"
    r = gone.track(*score._frame_at(torch.eye(4), 1))
    assert r.lost and score._ScoreMirrorMap.log == [] and r.weak is None


def test_the_option_of_the_evaluation_driver_needs_the_map_mode(tmp_path, capsys):
    from gsplatloc_amd import eval as ev

    with pytest.raises(ValueError, match="map_info"):
        ev.evaluate_room(None, 200, 3, sequential=True, map_info=True)
    for extra in (["--map-info"], ["--sequential", "--map-info"]):
        with pytest.raises(SystemExit):
            ev.main(["--root", str(tmp_path)] + extra)
        assert "needs --map" in capsys.readouterr().err
