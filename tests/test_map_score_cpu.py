"""Pose scores and relocalisation (csrc/map_score.hip, GaussianMap.score_poses, MapConfig.reloc), the parts that need no
GPU: the mirror of the rule on hand-made cases, MapConfig, the candidate poses, the entry point against its prototype and
its argument checks, and Localizer(mode="map") with ``reloc`` around a stand-in tracker that answers its start pose, the
stand-in renderer of tests/test_map_cpu.py and a map whose device calls are the mirrors, and the register budget of the
kernel.

The hand-made cases: a 6x4 image, the identity pose, intrinsics (4, 4, 2, 1) -- u = 4 x / z + 2, v = 4 y / z + 1 -- dyadic
rows and keep = 0.9375, beyond = 1.0625, so that every product, quotient and sum of the rule is exact and a row sits
where the case says.

The flow cases: the 32x24 box room of gsplatloc_amd.synthetic.  Frame 0 is taken at the identity.  A camera that has
moved BACK by 0.4 m sees the far wall 0.4 m further away: from the old pose the map's rows on that wall lie in front of
what the frame observes (the rows on the side walls, floor and ceiling still agree -- a ray that starts further back along
the optical axis meets them at the same depth), so the old pose is rejected, and the grid step "one reloc_trans back
along z" is the frame's pose exactly."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from gsplatloc_amd import _lib, mapping
from gsplatloc_amd.localizer import Localizer, LocalizeResult, reloc_candidates
from gsplatloc_amd.mapping import GaussianMap, MapConfig
from gsplatloc_amd.my_gsplat import TrackerConfig
from gsplatloc_amd.my_gsplat.trainer import TrackResult
from gsplatloc_amd.synthetic import replica_intrinsics, room_depth
from tests import map_score_ref as ref
from tests import test_map_cpu as base
from tests.test_abi import prototypes
from tests.test_kernel_resources import HIPCC, _resources

F32 = np.float32
RW, RH, INTR = 6, 4, (4.0, 4.0, 2.0, 1.0)
EYE = np.eye(4, dtype=F32)
KEEP, BEYOND = F32(0.9375), F32(1.0625)
NEAR = 0.25
SURFACE = np.full((RH, RW), 2.0, F32)  # a surface at 2 m everywhere: d * keep = 1.875, d * beyond = 2.125


def _p(u, v, z=1.0):
    """The row that projects onto (u, v) at depth z (exact for dyadic u, v, z)."""
    return [(u - 2.0) / 4.0 * z, (v - 1.0) / 4.0 * z, z]


def _verdict(point, depth=SURFACE, w2c=EYE, near=NEAR):
    """'untested' / 'front' / 'agree' / 'behind' of one row, and that exactly one of them holds."""
    t, a, f, b = (bool(m[0]) for m in ref.verdicts(np.array(point, F32).reshape(1, 3), w2c, INTR, depth, KEEP, BEYOND, near))
    assert (t, int(a) + int(f) + int(b)) in ((True, 1), (False, 0))
    return "untested" if not t else "front" if f else "agree" if a else "behind"


def _with(depth, **pixels):
    d = np.array(depth, F32).copy()
    for at, value in pixels.items():
        d[int(at[2]), int(at[1])] = value  # "p32" = column 3, line 2
    return d


# ---- the mirror of the rule -----------------------------------------------------------------------------------------
def test_rule_one_row_per_outcome():
    assert _verdict(_p(3, 2, 1.0)) == "front" and _verdict(_p(3, 2, 2.0)) == "agree" and _verdict(_p(3, 2, 4.0)) == "behind"
    # untested, each reason alone: behind the camera, on the near plane, outside the image on each of the four sides
    assert _verdict([0.25, 0.25, -1.0]) == "untested" and _verdict([0.0, 0.0, NEAR]) == "untested"
    assert _verdict([0.0, 0.0, float(np.nextafter(F32(NEAR), F32(9)))]) == "front"
    for outside in (_p(-1, 2), _p(6, 2), _p(3, -1), _p(3, 4)):
        assert _verdict(outside) == "untested"
    # the row's own pixel has no depth; its neighbours' depths are not looked at
    for bad in (0.0, -0.0, -1.0, np.nan, np.inf, -np.inf):
        assert _verdict(_p(3, 2, 2.0), _with(SURFACE, p32=bad)) == "untested"
        assert _verdict(_p(3, 2, 2.0), _with(SURFACE, p22=bad, p42=bad, p31=bad, p33=bad)) == "agree"
    # NaN / inf rows
    nan, inf = np.nan, np.inf
    for row in ([nan, 0.0, 1.0], [0.0, nan, 1.0], [0.0, 0.0, nan], [inf, 0.0, 1.0], [0.0, -inf, 1.0], [0.0, 0.0, inf],
                [0.0, 0.0, -inf], [nan, nan, nan]):
        assert _verdict(row) == "untested"
    # the pose counts: from a camera 1.5 m further back a row at 1 m lies behind the surface at 2 m
    moved = EYE.copy()
    moved[2, 3] = 1.5
    assert _verdict([0.0, 0.0, 1.0], w2c=moved) == "behind" and _verdict([0.0, 0.0, 0.5], w2c=moved) == "agree"


def test_rule_both_boundaries_agree():
    """z == d * keep and z == d * beyond (the float32 products) agree; one float32 step outside either does not."""
    lo, hi = F32(2.0) * KEEP, F32(2.0) * BEYOND
    assert float(lo) == 1.875 and float(hi) == 2.125
    assert _verdict(_p(3, 2, float(lo))) == "agree" and _verdict(_p(3, 2, float(np.nextafter(lo, F32(0))))) == "front"
    assert _verdict(_p(3, 2, float(hi))) == "agree" and _verdict(_p(3, 2, float(np.nextafter(hi, F32(9))))) == "behind"
    # the products are float32's: with rho = 0.05 neither 1 - rho nor 1 + rho is a float32 number
    k, b = ref.keep_of(0.05), ref.beyond_of(0.05)
    assert k.dtype == b.dtype == F32 and float(b) != 1.05 and float(F32(2.0) * b) != 2.0 * 1.05
    row = np.array([_p(3, 2, float(F32(2.0) * b)), _p(3, 2, float(np.nextafter(F32(2.0) * b, F32(9))))], F32)
    _, agree, _, behind = ref.verdicts(row, EYE, INTR, SURFACE, k, b, NEAR)
    assert agree.tolist() == [True, False] and behind.tolist() == [False, True]


def test_rule_rounds_half_to_even_and_minus_zero_is_column_zero():
    """The pixel a row is held against is rint's: u = 2.5 is column 2, 3.5 is column 4, -0.5 is column 0; u = W - 0.5
    rounds to W and is outside."""
    near_px = lambda c, r=1: _with(SURFACE, **{f"p{c}{r}": 0.5})  # noqa: E731  a surface at 0.5 m in that pixel only
    assert _verdict(_p(2.5, 1), near_px(2)) == "behind" and _verdict(_p(2.5, 1), near_px(3)) == "front"
    assert _verdict(_p(3.5, 1), near_px(4)) == "behind" and _verdict(_p(3.5, 1), near_px(3)) == "front"
    assert _verdict(_p(2, 0.5), near_px(2, 0)) == "behind" and _verdict(_p(2, 1.5), near_px(2, 2)) == "behind"
    on = _p(-0.5, 1)
    off = [float(np.nextafter(F32(on[0]), F32(-9))), on[1], 1.0]
    assert _verdict(on) == "front" and _verdict(on, near_px(0)) == "behind" and _verdict(off) == "untested"
    assert _verdict(_p(2, -0.5)) == "front" and _verdict(_p(5.5, 1)) == "untested" and _verdict(_p(2, 3.5)) == "untested"


def test_score_counts_per_pose():
    rows = np.array([_p(3, 2, 1.0), _p(3, 2, 2.0), _p(1, 1, 2.0), _p(3, 2, 4.0), _p(-1, 2), [np.nan, 0.0, 1.0]], F32)
    back = EYE.copy()
    back[2, 3] = 1.0  # the camera 1 m further back: depths 2, 3, 3, 5 against 2 m, and the row at u = -1 is in the
    away = EYE.copy()  # image now, at 2 m
    away[2, 3] = -9.0  # every row behind the camera
    got = ref.score(rows, np.stack([EYE, back, away]), INTR, SURFACE, KEEP, BEYOND, NEAR)
    assert got.dtype == np.int64 and got.shape == (3, 3)
    assert got.tolist() == [[4, 2, 1], [5, 2, 0], [0, 0, 0]]
    assert ref.score(rows[:0], EYE[None], INTR, SURFACE, KEEP, BEYOND, NEAR).tolist() == [[0, 0, 0]]


# ---- MapConfig ------------------------------------------------------------------------------------------------------
def test_map_config_validation():
    c = MapConfig()
    assert (c.reloc, c.reloc_min_tested, c.reloc_rot_deg, c.reloc_trans, c.reloc_levels) == (False, None, 2.0, 0.05, 2)
    assert 0.0 < c.reloc_min_agree <= 1.0
    ok = MapConfig(reloc=True, reloc_min_agree=1.0, reloc_min_tested=1, reloc_rot_deg=0.5, reloc_trans=1e-3, reloc_levels=1)
    assert ok.reloc and ok.reloc_levels == 1 and MapConfig(reloc=True, depth_rho=0.0).reloc
    bad = dict(reloc=[1, "yes", None, 0.5],
               reloc_min_agree=[0.0, -0.1, 1.0000001, float("nan"), True, "0.8", None],
               reloc_min_tested=[0, -3, 1.5, True, "7"],
               reloc_rot_deg=[0.0, -1.0, float("inf"), float("nan"), True, None],
               reloc_trans=[0.0, -0.05, float("inf"), float("nan"), False, None],
               reloc_levels=[0, 3, 1.0, True, None])
    for field, values in bad.items():
        for v in values:
            with pytest.raises(ValueError, match=field):
                MapConfig(**{field: v})
    for rho in (1.0, -0.01, 1.5):
        with pytest.raises(ValueError, match="depth_rho"):
            MapConfig(reloc=True, depth_rho=rho)
        assert MapConfig(depth_rho=rho).depth_rho == rho  # only the option needs it


# ---- the candidate poses --------------------------------------------------------------------------------------------
def _base(seed):
    from tests.pose_ref import axis_angle

    c2w = torch.eye(4)
    c2w[:3, :3] = axis_angle((0.4, -0.7, 0.6), 37.0 + seed).float()
    c2w[:3, 3] = torch.tensor([1.3, -0.8, 2.1 + seed])
    return c2w


def test_reloc_candidates_count_order_and_composition():
    b0, b1 = _base(0), _base(1)
    for levels in (1, 2):
        per = 1 + 12 * levels
        one, two = reloc_candidates([b0], 2.0, 0.05, levels), reloc_candidates([b0, b1], 2.0, 0.05, levels)
        assert one.shape == (per, 4, 4) and two.shape == (2 * per, 4, 4) and one.dtype == torch.float32
        assert torch.equal(two[:per], one) and torch.equal(one[0], b0) and torch.equal(two[per], b1)  # bit for bit
        rel = torch.linalg.inv(b0.double()) @ one.double()  # the steps in the camera's own frame
        k = 1
        for level in range(1, levels + 1):  # the turns: level, axis x y z, + then -
            for axis in range(3):
                for sign in (1.0, -1.0):
                    R = rel[k, :3, :3]
                    angle = np.degrees(np.arccos(np.clip((float(R.trace()) - 1.0) / 2.0, -1.0, 1.0)))
                    a, b = (axis + 1) % 3, (axis + 2) % 3
                    assert abs(angle - 2.0 * level) < 1e-3 and abs(float(R[axis, axis]) - 1.0) < 1e-6, (k, angle)
                    assert np.sign(float(R[b, a])) == sign and float(rel[k, :3, 3].abs().max()) < 1e-6, k
                    k += 1
        for level in range(1, levels + 1):  # the shifts
            for axis in range(3):
                for sign in (1.0, -1.0):
                    want = torch.zeros(3, dtype=torch.float64)
                    want[axis] = sign * level * 0.05
                    assert float((rel[k, :3, 3] - want).abs().max()) < 1e-6, k
                    assert float((rel[k, :3, :3] - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-6, k
                    k += 1
        assert k == per
    # a level-2 turn is two level-1 turns
    c = reloc_candidates([b0], 2.0, 0.05, 2).double()
    inv = torch.linalg.inv(b0.double())
    for j in range(6):
        assert float((c[7 + j] - c[1 + j] @ inv @ c[1 + j]).abs().max()) < 1e-6, j


def test_reloc_candidates_refuses_more_than_one_call_scores():
    bases = [_base(i) for i in range(6)]
    assert reloc_candidates(bases[:2], 2.0, 0.05, 2).shape[0] == 50
    assert reloc_candidates(bases[:4], 2.0, 0.05, 1).shape[0] == 52
    for n, levels in ((3, 2), (5, 1), (6, 2)):
        with pytest.raises(ValueError, match="64"):
            reloc_candidates(bases[:n], 2.0, 0.05, levels)
    with pytest.raises(ValueError, match=r"\(4, 4\)"):
        reloc_candidates([torch.eye(3)], 2.0, 0.05, 1)


# ---- the entry point ------------------------------------------------------------------------------------------------
BAD_ARG = -1
FN = "gsl_map_score"
GOOD = dict(n_rows=1000, n_poses=3, fx=50.0, fy=40.0, cx=31.5, cy=23.5, width=64, height=48, keep=0.95, beyond=1.05,
            near_plane=0.01)
REFUSED = [
    ("NULL means", dict(means=None)), ("NULL w2c", dict(w2c=None)), ("NULL depth", dict(depth=None)),
    ("NULL counts", dict(counts=None)), ("n_rows == 0", dict(n_rows=0)), ("n_rows < 0", dict(n_rows=-5)),
    ("n_rows == 2^31", dict(n_rows=1 << 31)), ("n_rows beyond 2^32", dict(n_rows=(1 << 32) + 7)),
    ("n_poses == 0", dict(n_poses=0)), ("n_poses < 0", dict(n_poses=-1)), ("n_poses == 65", dict(n_poses=65)),
    ("width <= 0", dict(width=0)), ("height <= 0", dict(height=-3)), ("2^31 pixels", dict(width=65536, height=32768)),
    ("fx == 0", dict(fx=0.0)), ("fy == 0", dict(fy=0.0)), ("fx == -0", dict(fx=-0.0)),
    ("keep == 0", dict(keep=0.0)), ("keep < 0", dict(keep=-0.5)), ("keep > 1", dict(keep=1.0000001)),
    ("NaN keep", dict(keep=float("nan"))), ("beyond < 1", dict(beyond=0.9999999)), ("beyond < 0", dict(beyond=-2.0)),
    ("NaN beyond", dict(beyond=float("nan"))),
]


def call_with(lib, params, named, pointers):
    """gsl_map_score with the named arguments over GOOD; ``pointers``: parameter name -> address."""
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
    """The prototype of include/gsloc_hip.h, the row of _lib._SIGNATURES (tests/test_abi.py compares the types) and the
    definition in csrc/map_score.hip: the same parameters, by type and name, in the same order; the pose limit is one
    number everywhere."""
    ret, params = prototypes(repo_root)[FN]
    assert ret == "int" and [n for _, n in params] == [
        "means", "n_rows", "w2c", "n_poses", "fx", "fy", "cx", "cy", "depth", "width", "height", "keep", "beyond",
        "near_plane", "counts", "stream"]
    assert len(_lib._SIGNATURES[FN][1]) == len(params)
    src = open(os.path.join(repo_root, "gsplatloc_amd", "csrc", "map_score.hip")).read()
    m = re.search(r'extern "C" int gsl_map_score\((.*?)\)\s*\{', src, flags=re.S)
    assert m, "no definition of gsl_map_score"
    defined = [re.fullmatch(r"\s*(.*?)\s*(\w+)\s*", p, flags=re.S).groups() for p in m.group(1).split(",")]
    assert [(" ".join(t.split()), n) for t, n in defined] == params
    assert prototypes(repo_root)["gsl_map_score_max_poses"] == ("int", [])
    header = open(os.path.join(repo_root, "include", "gsloc_hip.h")).read()
    limit = int(re.search(r"#define GSL_MAP_SCORE_MAX_POSES (\d+)", header).group(1))
    assert limit == 64 == mapping.SCORE_MAX_POSES == _lib.load_library().gsl_map_score_max_poses()
    assert "map_score.hip" in open(os.path.join(repo_root, "gsplatloc_amd", "csrc", "Makefile")).read()


def test_entry_point_rejects_bad_arguments_before_any_launch(repo_root):
    """Every row is refused on the host: the pointers are one dummy HOST buffer, a launch (the zeroing of counts is
    one) would give GSL_ERR_HIP or worse."""
    lib = _lib.load_library()
    params = prototypes(repo_root)[FN][1]
    buf = ctypes.create_string_buffer(b"\x7f" * 1024, 1024)
    pointers = {n: ctypes.addressof(buf) for t, n in params if "*" in t}
    for what, over in REFUSED:
        named = dict(GOOD, **over)
        assert set(named) <= {n for _, n in params}, what
        assert call_with(lib, params, named, pointers) == BAD_ARG, what
    assert buf.raw == b"\x7f" * 1024  # nothing wrote to the buffer


# ---- GaussianMap.score_poses and Localizer(mode="map", reloc) around the mirror -------------------------------------
W, H = base.W, base.H
CFG_NEAR = TrackerConfig().gs.near_plane
STEP = 0.4  # metres: the move of the flow cases and the translation step of their grid


class _ScoreMirrorMap(base._MirrorMap):
    """GaussianMap whose device calls are the numpy mirrors; records what it was asked to score and what it inserted."""
    log = []

    def _launch(self, depth, rgb, intr, c2w, render, alphas):
        _ScoreMirrorMap.log.append(dict(call="insert", c2w=c2w.clone()))
        return super()._launch(depth, rgb, intr, c2w, render, alphas)

    def _score_launch(self, depth, intr, w2c, near):
        counts = ref.score(self.means[:self.n_live].numpy(), w2c.numpy(), intr, depth.numpy(), F32(self.keep),
                           F32(self.beyond), near)
        _ScoreMirrorMap.log.append(dict(call="score", w2c=w2c.numpy().copy(), depth=depth.clone(), near=near,
                                        rows=self.n_live, counts=counts))
        return counts


class _StartTracker(base._Tracker):
    """Stands in for GraphTracker: run() answers the pose it was started from."""

    def run(self):
        start = self.loads[-1]["tar_c2w"]
        return TrackResult(best_loss=0.25, steps=12, final_c2w=start.clone(), best_c2w=start.clone(),
                           best_step=type(self).best_step)


class _StartTrackerWithoutMinimum(_StartTracker):
    best_step = -1


def _shift(axis, metres):
    c2w = torch.eye(4)
    c2w[axis, 3] = metres
    return c2w


def _frame_at(c2w, seed=0):
    K = replica_intrinsics(W, H)
    rgb = torch.randint(0, 255, (H, W, 3), generator=torch.Generator().manual_seed(seed)).float()
    return room_depth(W, H, K, c2w), rgb


def _localizer(tracker, monkeypatch, **cfg):
    import gsplatloc_amd.data.dataset as DS

    monkeypatch.setattr(DS, "compute_depth_gt", lambda pts, col, Ks, c2w, height, width: torch.zeros(height, width))
    tracker.made = base._Tracker.made = []
    loc = Localizer(replica_intrinsics(W, H), W, H, TrackerConfig(max_steps=5), normalize=False, motion="hold",
                    device="cpu", tracker_factory=tracker, mode="map", map_factory=_ScoreMirrorMap,
                    map_renderer=base._Renderer(), map_config=MapConfig(**cfg))
    loc.reset(*_frame_at(torch.eye(4)), torch.eye(4))
    _ScoreMirrorMap.log = []
    return loc


def _scores(loc, depth, poses):
    """The mirror on host copies, called by the test itself."""
    w2cs = np.stack([ref.w2c_of(p.numpy()) for p in poses])
    K = replica_intrinsics(W, H)
    intr = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
    return ref.score(loc.map.points.numpy(), w2cs, intr, depth.numpy(), F32(loc.map.keep), F32(loc.map.beyond), CFG_NEAR)


def test_score_poses_hands_the_mirror_what_the_kernel_gets():
    m = _ScoreMirrorMap(W, H, MapConfig(depth_rho=0.05), "cpu")
    _ScoreMirrorMap.log = []
    K, (depth, rgb) = replica_intrinsics(W, H), _frame_at(torch.eye(4))
    assert m.score_poses(depth, K, [torch.eye(4)] * 3, CFG_NEAR).tolist() == [[0, 0, 0]] * 3  # an empty map: no call
    assert _ScoreMirrorMap.log == [] and m.keep == float(ref.keep_of(0.05)) and m.beyond == float(ref.beyond_of(0.05))
    m.insert_frame(depth, rgb, K, torch.eye(4))
    poses = torch.stack([torch.eye(4), _shift(2, -STEP), _base(0)])
    got = m.score_poses(depth, K, poses, CFG_NEAR)
    assert got.dtype == np.int64 and got.shape == (3, 3) and got[0].tolist() == [W * H, W * H, 0]
    assert got[1, 0] == W * H and 0 < got[1, 1] < W * H and got[1, 2] == 0  # from further back the far wall is BEHIND
    call = _ScoreMirrorMap.log[-1]
    assert call["near"] == CFG_NEAR and call["rows"] == W * H and call["w2c"].dtype == F32
    for k in range(3):  # the float64 inverse, rounded to float32 once
        assert np.array_equal(call["w2c"][k], ref.w2c_of(poses[k].numpy()))
    assert np.array_equal(m.score_poses(depth, K, list(poses), CFG_NEAR), got)  # a sequence of poses is the same
    with pytest.raises(ValueError, match="64"):
        m.score_poses(depth, K, [torch.eye(4)] * 65, CFG_NEAR)
    with pytest.raises(ValueError, match=r"\(4, 4\)"):
        m.score_poses(depth, K, [torch.eye(4), torch.eye(3)], CFG_NEAR)
    with pytest.raises(ValueError, match="depth"):
        m.score_poses(torch.ones(H, W + 1), K, [torch.eye(4)], CFG_NEAR)
    host = GaussianMap(W, H, MapConfig(), "cpu")
    host.n_live = 3
    with pytest.raises(AssertionError, match="no CPU path"):
        host.score_poses(depth, K, [torch.eye(4)], CFG_NEAR)


def test_an_accepted_estimate_is_scored_once_and_not_tracked_again(monkeypatch):
    loc = _localizer(_StartTracker, monkeypatch, reloc=True)
    depth, rgb = _frame_at(torch.eye(4), 1)
    r = loc.track(depth, rgb, gt_c2w=torch.eye(4))
    assert [c["call"] for c in _ScoreMirrorMap.log] == ["score", "insert"]  # scored before anything touches the map
    call = _ScoreMirrorMap.log[0]
    assert call["w2c"].shape == (1, 4, 4) and torch.equal(call["depth"], depth) and call["near"] == CFG_NEAR
    assert (r.lost, r.relocalised, r.tested, r.agree, r.front) == (False, False, W * H, W * H, 0)
    assert len(_StartTracker.made) == 1 and len(_StartTracker.made[0].loads) == 1 and r.steps == 12
    assert r.added == H and r.map_size == W * H + H and torch.equal(r.c2w, torch.eye(4))


def test_a_rejected_estimate_is_tracked_again_from_the_mirrors_winner(monkeypatch):
    loc = _localizer(_StartTracker, monkeypatch, reloc=True, reloc_trans=STEP, reloc_rot_deg=3.0)
    truth = _shift(2, -STEP)
    depth, rgb = _frame_at(truth, 1)
    cands = reloc_candidates([torch.eye(4)], 3.0, STEP, 2)
    want = _scores(loc, depth, list(cands))
    margins = (want[:, 1] - want[:, 2]).tolist()
    winner = margins.index(max(margins))
    assert torch.equal(cands[winner], truth) and winner == 1 + 12 + 5  # one step back along z: the frame's own pose
    assert want[winner].tolist() == [W * H, W * H, 0] and sorted(margins)[-2] < W * H
    # the far wall's rows are in front of what the frame sees: the start is rejected
    assert want[0, 1] < MapConfig().reloc_min_agree * (want[0, 1] + want[0, 2])
    r = loc.track(depth, rgb, gt_c2w=truth)
    assert [c["call"] for c in _ScoreMirrorMap.log] == ["score", "score", "score", "insert"]
    first, grid, second, insert = _ScoreMirrorMap.log
    assert first["counts"].tolist() == [want[0].tolist()] and np.array_equal(grid["counts"], want)
    assert np.array_equal(grid["w2c"], np.stack([ref.w2c_of(c.numpy()) for c in cands]))  # one call for the whole grid
    assert np.array_equal(second["w2c"][0], ref.w2c_of(truth.numpy())) and grid["rows"] == second["rows"] == W * H
    # tracked again, from the winner; its answer is accepted, and its rows go in at that pose
    loads = [load for t in _StartTracker.made for load in t.loads]
    assert len(loads) == 2 and torch.equal(loads[0]["tar_c2w"], torch.eye(4)) and torch.equal(loads[1]["tar_c2w"], truth)
    assert (r.lost, r.relocalised, r.steps, r.best_step) == (False, True, 24, _StartTracker.best_step)
    assert (r.tested, r.agree, r.front) == (W * H, W * H, 0) and torch.equal(r.c2w, truth) and r.eT == 0.0
    assert torch.equal(r.init_c2w, truth) and torch.equal(insert["c2w"], truth) and torch.equal(loc.trajectory[-1], truth)
    assert r.added == H and r.map_size == W * H + H == loc.map.n_live


@pytest.mark.parametrize("why", ["no minimum", "too few rows"])
def test_a_winner_that_is_the_failed_start_gives_a_lost_frame(monkeypatch, why):
    """The start agrees with every row and still is not accepted -- the tracker recorded no minimum, or fewer rows were
    tested than asked for: no candidate scores higher, index 0 wins the tie, and nothing is tracked again."""
    tracker = _StartTrackerWithoutMinimum if why == "no minimum" else _StartTracker
    loc = _localizer(tracker, monkeypatch, reloc=True, **({} if why == "no minimum" else dict(reloc_min_tested=W * H + 1)))
    before = loc.map.points.clone()
    r = loc.track(*_frame_at(torch.eye(4), 1))
    assert [(c["call"], len(c["w2c"])) for c in _ScoreMirrorMap.log] == [("score", 1), ("score", 25)]
    margins = (_ScoreMirrorMap.log[1]["counts"][:, 1] - _ScoreMirrorMap.log[1]["counts"][:, 2]).tolist()
    assert margins.index(max(margins)) == 0 and margins[0] == W * H
    assert (r.lost, r.relocalised, r.steps) == (True, False, 12) and (r.tested, r.agree, r.front) == (W * H, W * H, 0)
    assert len(tracker.made) == 1 and len(tracker.made[0].loads) == 1
    assert r.added == 0 and r.map_size == W * H == loc.map.n_live and torch.equal(loc.map.points, before)
    assert loc.trajectory.shape == (2, 4, 4) and torch.equal(r.c2w, torch.eye(4))


def test_a_rejected_second_run_gives_a_lost_frame_with_the_better_pose(monkeypatch):
    """More rows are asked for than the map has: the second estimate, the frame's own pose, is rejected as well.  The
    frame is lost, the map is left alone, and of the two estimates the one with the larger agree - front is kept."""
    loc = _localizer(_StartTracker, monkeypatch, reloc=True, reloc_trans=STEP, reloc_min_tested=W * H + 1)
    truth = _shift(2, -STEP)
    depth, rgb = _frame_at(truth, 1)
    before = loc.map.points.clone()
    r = loc.track(depth, rgb, gt_c2w=truth)
    assert [(c["call"], len(c["w2c"])) for c in _ScoreMirrorMap.log] == [("score", 1), ("score", 25), ("score", 1)]
    first, second = _ScoreMirrorMap.log[0]["counts"][0], _ScoreMirrorMap.log[2]["counts"][0]
    assert second[1] - second[2] > first[1] - first[2]
    assert (r.lost, r.relocalised, r.steps) == (True, False, 24) and torch.equal(r.c2w, truth)
    assert (r.tested, r.agree, r.front) == tuple(second.tolist()) == (W * H, W * H, 0)
    assert sum(len(t.loads) for t in _StartTracker.made) == 2
    assert r.added == 0 and r.map_size == W * H == loc.map.n_live and torch.equal(loc.map.points, before)
    assert torch.equal(loc.trajectory[-1], truth)


def test_without_reloc_nothing_is_scored(monkeypatch):
    loc = _localizer(_StartTracker, monkeypatch)
    r = loc.track(*_frame_at(_shift(2, -STEP), 1))
    assert [c["call"] for c in _ScoreMirrorMap.log] == ["insert"] and loc.map._score is None
    assert (r.relocalised, r.tested, r.agree, r.front, r.lost) == (None, None, None, None, False)
    assert LocalizeResult(torch.eye(4), torch.eye(4), 1, 1, 0.0, False).relocalised is None


def test_the_options_of_the_evaluation_driver_need_the_map_mode(tmp_path, capsys):
    from gsplatloc_amd import eval as ev

    with pytest.raises(ValueError, match="map_reloc"):
        ev.evaluate_room(None, 200, 3, sequential=True, map_reloc=True)
    with pytest.raises(ValueError, match="map_reloc"):
        ev.evaluate_room(None, 200, 3, sequential=True, map_mode=True, map_reloc_trans=0.1)
    for extra, needs in ((["--map-reloc"], "--map"), (["--sequential", "--map-reloc"], "--map"),
                         (["--map-reloc-min-agree", "0.7"], "--map"),
                         (["--sequential", "--map", "--map-reloc-rot-deg", "1"], "--map-reloc"),
                         (["--sequential", "--map", "--map-reloc-trans", "0.1"], "--map-reloc")):
        with pytest.raises(SystemExit):
            ev.main(["--root", str(tmp_path)] + extra)
        assert f"needs {needs}" in capsys.readouterr().err


# ---- the kernel's budget --------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_the_score_kernel_stays_in_registers():
    """k_map_score: no scratch, no accumulation registers, the [64][3] table of counts in LDS, eight waves per SIMD."""
    hit = [v for k, v in _resources("map_score.hip").items() if "k_map_score" in k]
    assert len(hit) == 1
    r = hit[0]
    assert r["ScratchSize"] == 0 and r["Occupancy"] == 8 and r["AGPRs"] == 0 and r["LDS"] == 3 * 64 * 4, r
