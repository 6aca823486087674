"""Trajectory correction (csrc/map_correct.hip, GaussianMap.origins / correct / rows_up_to / loop_constraint,
mapping.spread_correction, Localizer.correct_trajectory / close_loop), the parts that need no GPU: the mirror
tests/map_correct_ref.py clause by clause, ``spread_correction`` against a reference that takes the logarithm and the
exponential of a generic matrix, the drifting circle, the origins through every removal of a map whose device calls are
the mirrors, ``Localizer.close_loop`` around stand-ins, the entry point's argument checks and the kernel's registers.

The drifting circle: cameras evenly on a circle of radius 0.5 m looking outwards, 24 or 48 of them; the tracker's
trajectory starts at the first true pose and adds the same body-frame error to every motion (0.1 .. 0.5 degrees,
2 .. 10 mm); every frame writes 200 random camera points at 1 .. 3 m into the map at its DRIFTED pose, as float32 rows.
The one constraint is the true pose of the last frame.  An error that grows linearly along the path is removed by a
correction that grows linearly along the path, up to the second-order term of the drift's rotation: the RMS distance
of the rows from where the true poses put them has to fall to half or less (1.0: a correction that does nothing).
Measured on the mirror: 0.194 (24 frames, 0.1 degrees / 2 mm), 0.189 (24, 0.5 / 10), 0.180 (48, 0.5 / 10)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from gsplatloc_amd import _lib
from gsplatloc_amd.localizer import Localizer, TrajectoryCorrection
from gsplatloc_amd.mapping import GaussianMap, LoopConstraint, MapConfig, PoseAlignment, spread_correction
from gsplatloc_amd.my_gsplat import TrackerConfig
from gsplatloc_amd.my_gsplat.geometry import depth_to_points
from gsplatloc_amd.synthetic import replica_intrinsics, room_depth
from tests import map_correct_ref as ref
from tests import test_map_cpu as base
from tests import test_map_refine_cpu as refine_cpu
from tests.test_abi import prototypes
from tests.test_kernel_resources import HIPCC, _resources
from tests.test_map_cpu import sequence  # noqa: F401  (the 32x24 drifting sequence, a module fixture there)

F32 = np.float32
EYE12 = ref.IDENTITY


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _entry(R=None, t=(0.0, 0.0, 0.0)):
    e = np.zeros((3, 4), F32)
    e[:, :3] = np.eye(3) if R is None else R
    e[:, 3] = t
    return e.reshape(12)


QUARTER = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]  # a quarter turn about z: (x, y, z) -> (-y, x, z)


# ---- the mirror, clause by clause -----------------------------------------------------------------------------------
def test_a_moved_row():
    table = np.stack([EYE12, _entry(QUARTER, (0.5, -0.25, 2.0))])
    r = ref.correct([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0]], [0, 1], table)
    assert r["moved"].tolist() == [False, True] and r["counters"] == (1, 0)
    assert r["means"].tolist() == [[1.0, 2.0, 3.0], [-1.5, 0.75, 5.0]]
    # a pure translation is not the identity either, and neither is an entry that differs in one element only
    for j in range(12):
        e = EYE12.copy()
        e[j] = e[j] + F32(0.5)
        assert ref.correct([[1.0, 2.0, 3.0]], [0], e[None])["moved"].all(), j
    # float32, one rounding per operation, in the order ((r0 x + r1 y) + r2 z) + t
    e = _entry([[0.1, 0.7, -0.3], [0.2, 0.9, 0.4], [-0.6, 0.05, 0.8]], (0.01, 1e-3, -3.0))
    p = np.array([[1.7, -2.9, 0.33]], F32)
    got = ref.correct(p, [0], e[None])["means"][0]
    for a in range(3):
        w = e[4 * a:4 * a + 4]
        want = F32(F32(F32(F32(w[0] * p[0, 0]) + F32(w[1] * p[0, 1])) + F32(w[2] * p[0, 2])) + w[3])
        assert got[a] == want and got.dtype == F32


def test_an_identity_entry_keeps_every_bit():
    p = np.array([[-0.0, 1.0, -0.0], [3.0, -0.0, 0.0]], F32)
    for e in (EYE12, np.where(EYE12 == 0, F32(-0.0), EYE12)):  # -0.0 in the entry counts as 0
        r = ref.correct(p, [0, 0], e[None])
        assert not r["moved"].any() and r["counters"] == (0, 0) and np.array_equal(_bits(r["means"]), _bits(p))
    # the product the rule skips would have lost the sign: 1 * -0.0 + 0 * 1.0 = +0.0
    assert np.signbit(p[0, 0]) and not np.signbit(F32(1.0) * p[0, 0] + F32(0.0) * p[0, 1])
    # an entry with a NaN is not the identity: the row moves (to NaN -- the caller's table, the caller's result)
    e = EYE12.copy()
    e[3] = np.nan
    r = ref.correct([[1.0, 2.0, 3.0]], [0], e[None])
    assert r["moved"].all() and np.isnan(r["means"][0, 0]) and r["means"][0, 1:].tolist() == [2.0, 3.0]


def test_rows_that_are_not_numbers_and_origins_outside_the_table_are_left_alone():
    table = np.stack([_entry(QUARTER, (1.0, 1.0, 1.0))] * 3)
    nan, inf = np.nan, np.inf
    p = np.array([[nan, 0, 2], [0, nan, 2], [0, 0, nan], [inf, 0, 2], [0, -inf, 2], [0, 0, inf], [nan, inf, -inf]], F32)
    r = ref.correct(p, [1] * len(p), table)
    assert not r["moved"].any() and r["counters"] == (0, 0) and np.array_equal(_bits(r["means"]), _bits(p))
    q = np.array([[1.0, 2.0, 3.0]] * 5, F32)
    r = ref.correct(q, [-1, 3, 2, -2 ** 31, 2 ** 31 - 1], table)
    assert r["outside"].tolist() == [True, True, False, True, True] and r["moved"].tolist() == [False, False, True, False, False]
    assert r["counters"] == (1, 4) and np.array_equal(_bits(r["means"][[0, 1, 3, 4]]), _bits(q[[0, 1, 3, 4]]))
    # a row that is not a number AND outside the table counts as outside: the origin is looked at first
    assert ref.correct([[nan, 0, 0]], [7], table)["counters"] == (0, 1)


def test_counts():
    rng = np.random.default_rng(3)
    table = np.stack([EYE12, _entry(QUARTER), EYE12, _entry(None, (0.0, 0.0, 0.125))])
    o = np.sort(rng.integers(-1, 6, 500)).astype(np.int32)
    p = rng.uniform(-8, 8, (500, 3)).astype(F32)
    p[::50, 1] = np.nan
    r = ref.correct(p, o, table)
    inside = (o >= 0) & (o < 4)
    want_moved = inside & np.isin(o, (1, 3)) & np.isfinite(p).all(axis=1)
    assert r["counters"] == (int(want_moved.sum()), int((~inside).sum())) and np.array_equal(r["moved"], want_moved)
    assert np.array_equal(_bits(r["means"][~want_moved]), _bits(p[~want_moved]))
    assert ref.correct(np.zeros((0, 3), F32), np.zeros(0, np.int32), table)["counters"] == (0, 0)
    T = np.tile(np.eye(4), (2, 1, 1))
    T[1, :3, 3] = (0.1, 0.2, 0.3)
    assert ref.table_of(T).dtype == F32 and ref.table_of(T).shape == (2, 12)
    assert np.array_equal(ref.table_of(T)[0], EYE12) and ref.table_of(T)[1, 3] == F32(0.1)


# ---- spread_correction ----------------------------------------------------------------------------------------------
def _wander(n, seed=1):
    """[n,4,4] float64: a trajectory with steps of unequal length (so that "path" and "index" differ)."""
    rng = np.random.default_rng(seed)
    out = [np.eye(4)]
    for k in range(n - 1):
        out.append(out[-1] @ ref.twist(rng.uniform(0.0, 3.0), rng.uniform(0.0, 0.2), rng.normal(size=3), rng.normal(size=3)))
    return np.stack(out)


DELTA = ref.twist(7.0, 0.3, (0.2, -1.0, 0.4), (1.0, 0.5, -0.3))


def _rigid(T, tol=1e-12):
    R = T[:3, :3]
    return (np.abs(R.T @ R - np.eye(3)).max() <= tol and abs(np.linalg.det(R) - 1.0) <= tol
            and T[3].tolist() == [0.0, 0.0, 0.0, 1.0])


@pytest.mark.parametrize("by", ["path", "index"])
def test_spread_correction_against_the_generic_reference(by):
    poses = _wander(12)
    first, last = 2, 9
    D = spread_correction(poses, first, last, DELTA, by)
    want, s = ref.spread(poses, first, last, DELTA, by)
    assert D.shape == (12, 4, 4) and D.dtype == np.float64
    assert np.abs(D - want).max() <= 1e-12
    for k in range(first + 1):  # exactly the identity, not nearly: the rows of these frames keep their bits
        assert np.array_equal(D[k], np.eye(4)) and not np.signbit(D[k]).any()
    for k in range(last, 12):
        assert np.abs(D[k] - DELTA).max() <= 1e-12
    assert all(_rigid(D[k]) for k in range(12))
    # s_k is monotone: the angle and the translation of log(D_k) grow with k, and stay within delta's
    angle = np.degrees(np.arccos(np.clip((np.trace(D[:, :3, :3], axis1=1, axis2=2) - 1) / 2, -1, 1)))
    assert (np.diff(s) >= 0).all() and (np.diff(angle) >= -1e-9).all() and abs(angle[-1] - 7.0) <= 1e-9
    assert np.allclose(angle, 7.0 * s, atol=1e-6)
    if by == "index":
        assert np.allclose(s[first:last + 1], np.arange(8) / 7.0)
    else:
        assert np.abs(s[first:last + 1] - np.arange(8) / 7.0).max() > 0.02  # unequal steps: another spread


def test_spread_correction_without_a_path_falls_back_to_the_index():
    still = np.tile(ref.twist(10.0, 0.5), (6, 1, 1))  # the camera never moved
    D = spread_correction(still, 0, 5, DELTA)
    assert np.abs(D - ref.spread(still, 0, 5, DELTA, "index")[0]).max() <= 1e-12 and not np.array_equal(D[1], np.eye(4))
    # a tiny correction goes through the series of the closed form
    tiny = ref.twist(1e-6, 1e-7)
    D = spread_correction(_wander(5), 0, 4, tiny)
    assert np.abs(D[4] - tiny).max() <= 1e-15 and np.abs(D - ref.spread(_wander(5), 0, 4, tiny)[0]).max() <= 1e-12
    # the identity as the correction: nothing moves
    assert np.array_equal(spread_correction(_wander(5), 1, 3, np.eye(4)), np.tile(np.eye(4), (5, 1, 1)))
    # tensors and float32 poses are taken
    D32 = spread_correction(torch.from_numpy(_wander(5)).float(), 0, 4, torch.from_numpy(DELTA))
    assert np.abs(D32 - spread_correction(_wander(5), 0, 4, DELTA)).max() <= 1e-5


def test_spread_correction_commutes_with_a_change_of_the_world():
    """c2w' = T c2w and delta' = T delta T^-1 describe the same cameras and the same correction in another world frame:
    D_k' = T D_k T^-1."""
    poses, T = _wander(10, seed=4), ref.twist(63.0, 1.7, (1.0, 0.2, 0.1), (-0.3, 0.2, 1.0))
    Ti = np.linalg.inv(T)
    for by in ("path", "index"):
        D = spread_correction(poses, 1, 8, DELTA, by)
        D2 = spread_correction(T @ poses, 1, 8, T @ DELTA @ Ti, by)
        assert np.abs(D2 - T @ D @ Ti).max() <= 1e-10


def test_spread_correction_refuses():
    poses = _wander(6)
    shear, mirror, scaled, open_row = DELTA.copy(), DELTA.copy(), DELTA.copy(), DELTA.copy()
    shear[0, 1] += 0.01
    mirror[:3, 0] *= -1.0
    scaled[:3, :3] *= 1.001
    open_row[3, 0] = 0.1
    nan = DELTA.copy()
    nan[1, 3] = np.nan
    bad = [dict(first=3, last=3), dict(first=4, last=2), dict(first=-1), dict(last=6), dict(first=1.5), dict(last=True),
           dict(delta=shear), dict(delta=mirror), dict(delta=scaled), dict(delta=open_row), dict(delta=nan),
           dict(delta=np.eye(3)), dict(delta=ref.twist(90.0, 0.0)), dict(delta=ref.twist(135.0, 0.1)),
           dict(delta=ref.twist(180.0, 0.0)), dict(by="time"), dict(poses=poses[:, :3])]
    for over in bad:
        a = dict(dict(poses=poses, first=1, last=4, delta=DELTA, by="path"), **over)
        with pytest.raises(ValueError):
            spread_correction(a["poses"], a["first"], a["last"], a["delta"], a["by"])
    assert spread_correction(poses, 0, 5, ref.twist(89.9, 0.0)).shape == (6, 4, 4)  # just below a quarter turn


# ---- the drifting circle --------------------------------------------------------------------------------------------
CIRCLES = [(24, 0.1, 0.002), (24, 0.5, 0.010), (48, 0.5, 0.010)]


def circle_rows(n, rot_deg, trans, per_frame=200):
    """(drifted poses, true poses, rows [n * per_frame, 3] float32 at the drifted poses, where the true poses put them
    [.., 3] float64, origins int32) -- ``default_rng(0)``."""
    rng = np.random.default_rng(0)
    true = ref.circle_poses(n, 0.5)
    est = ref.drifted(true, rot_deg, trans)
    z = rng.uniform(1.0, 3.0, (n, per_frame, 1))
    cam = np.concatenate([rng.uniform(-0.5, 0.5, (n, per_frame, 2)) * z, z, np.ones((n, per_frame, 1))], -1)
    rows = np.einsum("kij,knj->kni", est, cam)[..., :3].astype(F32).reshape(-1, 3)
    want = np.einsum("kij,knj->kni", true, cam)[..., :3].reshape(-1, 3)
    return est, true, rows, want, np.repeat(np.arange(n), per_frame).astype(np.int32)


@pytest.mark.parametrize("n,rot_deg,trans", CIRCLES)
@pytest.mark.parametrize("by", ["path", "index"])
def test_the_drifting_circle(n, rot_deg, trans, by):
    est, true, rows, want, origins = circle_rows(n, rot_deg, trans)
    D = spread_correction(est, 0, n - 1, true[-1] @ np.linalg.inv(est[-1]), by)
    r = ref.correct(rows, origins, ref.table_of(D))
    before, after = ref.rms(rows - want), ref.rms(r["means"].astype(np.float64) - want)
    print(f"[correct] circle of {n}, {rot_deg} deg / {trans * 1e3:g} mm a frame, by {by}: RMS {before:.4f} m -> "
          f"{after:.4f} m, x {after / before:.3f}")
    assert r["counters"] == (len(rows) - 200, 0)  # frame 0 stays: its D is the identity itself
    assert np.array_equal(_bits(r["means"][:200]), _bits(rows[:200]))
    assert after / before <= 0.5
    # ... and the corrected poses themselves: the last one is the constraint
    assert np.abs(D[-1] @ est[-1] - true[-1]).max() <= 1e-12


# ---- the origins on a map whose device calls are the mirrors ----------------------------------------------------------
W, H = base.W, base.H
K = replica_intrinsics(W, H)
NEAR = TrackerConfig().gs.near_plane


class _CorrectMirrorMap(refine_cpu._RefineMirrorMap):
    """The mirror map of the refinement tests; the three removals carry the origins as gsl_map_gather_i32 does (by the
    ids they stored), and ``correct``'s device call is the mirror."""

    def _stored(self, ids, means=None, colors=None, stamps=None):
        super()._stored(ids, means, colors, stamps)
        if self.origins is not None:
            self._free_buffers()["origins"][:len(ids)] = self.origins[torch.from_numpy(ids).long()]

    def _correct_launch(self, table):
        n = self.n_live
        assert table.dtype == torch.float32 and table.shape[1:] == (12,) and table.is_contiguous()
        r = ref.correct(self.means[:n].numpy(), self.origins[:n].numpy(), table.numpy())
        self._say("correct", table=table.numpy().copy(), moved=r["moved"])
        self.means[:n] = torch.from_numpy(r["means"])
        return r["counters"]


def _ordered(m):
    o = m.origins[:m.n_live].numpy()
    return bool((np.diff(o) >= 0).all())


def _prefixes_agree(m):
    o = m.origins[:m.n_live].numpy()
    frames = [-5, -1] + list(range(int(o.max()) + 3)) + [2 ** 31 - 1, 2 ** 40]
    return all(m.rows_up_to(f) == int((o <= f).sum()) for f in frames)


def test_without_the_option_there_are_no_origins():
    m = _CorrectMirrorMap(W, H, MapConfig(free_rho=0.05), "cpu")
    assert m.origins is None and m._free_buffers()["origins"] is None and MapConfig().origins is False
    depth, rgb = torch.full((H, W), 2.0), torch.full((H, W, 3), 100.0)
    assert m.insert_frame(depth, rgb, K, torch.eye(4), origin=-7) == (W * H, W * H)  # not looked at
    with pytest.raises(RuntimeError, match="origins"):
        m.rows_up_to(0)
    with pytest.raises(RuntimeError, match="origins"):
        m.correct(np.tile(np.eye(4), (2, 1, 1)))
    with pytest.raises(RuntimeError, match="origins"):
        m.loop_constraint(depth, K, torch.eye(4), 0, NEAR)
    for bad in (1, None, "yes"):
        with pytest.raises(ValueError, match="origins"):
            MapConfig(origins=bad)


def test_the_origins_follow_their_rows_and_stay_non_decreasing():
    cfg = MapConfig(origins=True, refine=True, free_rho=0.05, evict=True, merge_voxel=0.25, capacity=3 * W * H)
    m = _CorrectMirrorMap(W, H, cfg, "cpu")
    assert m.origins.shape == (m.capacity,) and m.origins.dtype == torch.int32 and m.rows_up_to(3) == 0
    m.origins[:] = 99
    depth, rgb = room_depth(W, H, K, torch.eye(4)), torch.full((H, W, 3), 100.0)
    render, alphas = torch.full((H, W), 0.01), torch.ones(H, W)
    alphas[:, 0] = 0.25  # H pixels are new per later frame
    assert m.insert_frame(depth, rgb, K, torch.eye(4)) == (W * H, W * H)  # default: the insertions since clear()
    assert (m.origins[:W * H] == 0).all() and (m.origins[W * H:] == 99).all()
    assert m.insert_frame(depth, rgb, K, torch.eye(4), render, alphas) == (H, H)  # ... 1
    assert m.insert_frame(depth, rgb, K, torch.eye(4), render, alphas, origin=4) == (H, H)
    assert m.insert_frame(depth, rgb, K, torch.eye(4), render, alphas, origin=4) == (H, H)  # equal is allowed
    assert m.insert_frame(depth, rgb, K, torch.eye(4), render, alphas, origin=np.int64(9)) == (H, H)
    n = m.n_live
    assert n == W * H + 4 * H
    assert m.origins[:n].tolist() == [0] * (W * H) + [1] * H + [4] * (2 * H) + [9] * H
    assert _ordered(m) and _prefixes_agree(m) and m.rows_up_to(3) == W * H + H and m.rows_up_to(8) == n - H
    # a decreasing origin, a negative one, one that is no index: refused before any launch, nothing changes
    calls = len(refine_cpu._RefineMirrorMap.log)
    for bad in (8, 0, -1, 2 ** 31, 1.0, True, "3"):
        with pytest.raises(ValueError, match="origin"):
            m.insert_frame(depth, rgb, K, torch.eye(4), render, alphas, origin=bad)
    with pytest.raises(ValueError, match="origin"):  # the default, five insertions so far, lies below 9 as well
        m.insert_frame(depth, rgb, K, torch.eye(4), render, alphas)
    assert len(refine_cpu._RefineMirrorMap.log) == calls and m.n_live == n and m._last_origin == 9
    # free space: a block of frame 0's rows and half of frame 4's, pulled to half their distance, go
    old_o, old_w = m.origins[:n].clone(), m.weights[:n].clone()
    block = torch.zeros(n, dtype=torch.bool)
    block[:W * H] = torch.zeros(H, W, dtype=torch.bool).index_fill_(0, torch.arange(8, 16), True).reshape(-1) \
        & torch.zeros(H, W, dtype=torch.bool).index_fill_(1, torch.arange(10, 20), True).reshape(-1)
    block[W * H + H:W * H + 2 * H] = True
    m.means[:n][block] *= 0.5
    optr = m.origins.data_ptr()
    removed, kept = m.remove_seen_through(depth, K, torch.eye(4), NEAR)
    assert removed >= 80 and kept == n - removed and m.origins.data_ptr() != optr
    assert m._free["origins"].data_ptr() == optr
    ids = m.survivors.long()
    assert torch.equal(m.origins[:kept], old_o[ids]) and torch.equal(m.weights[:kept], old_w[ids])
    assert _ordered(m) and _prefixes_agree(m)
    # eviction: the least recently observed rows go, wherever they came from
    n, old_o = kept, m.origins[:kept].clone()
    m.stamps[:n], m.frame_index = (torch.arange(n, dtype=torch.int32) * 7) % 5, 5
    evicted, kept = m.evict(150)
    ids = m.survivors.long()
    assert evicted == 150 and kept == n - 150 and torch.equal(m.origins[:kept], old_o[ids])
    assert len(set(old_o[ids].tolist())) == 4 and _ordered(m) and _prefixes_agree(m)
    # merge: a fused voxel keeps the origin of the row that stays, the first in map order
    n, old_o = kept, m.origins[:kept].clone()
    removed, kept = m.merge()
    ids = m.survivors.long()
    assert removed > 100 and kept == n - removed and torch.equal(m.origins[:kept], old_o[ids])
    assert _ordered(m) and _prefixes_agree(m)
    # nothing goes: nothing is swapped
    optr = m.origins.data_ptr()
    assert m.merge() == (0, kept) and m.origins.data_ptr() == optr
    # an insertion after the removals goes to the end; refinement leaves the origins alone
    before = m.origins[:kept].clone()
    assert m.refine(depth, None, K, torch.eye(4), NEAR) > 0 and torch.equal(m.origins[:kept], before)
    assert m.insert_frame(depth, rgb, K, torch.eye(4), render, alphas, origin=12)[1] == H
    assert (m.origins[kept:kept + H] == 12).all() and _ordered(m) and _prefixes_agree(m)
    # clear() starts over: the default is 0 again
    m.clear()
    assert m.insert_frame(depth, rgb, K, torch.eye(4))[1] == W * H and (m.origins[:W * H] == 0).all()
    assert m.rows_up_to(0) == W * H and m.rows_up_to(-1) == 0


def test_correct_on_the_map():
    cfg = MapConfig(origins=True, reloc=True, keyframes=True, keyframe_trans=0.01, capacity=W * H + 4 * H)
    m = _CorrectMirrorMap(W, H, cfg, "cpu")
    refine_cpu._RefineMirrorMap.log = []
    assert m.correct(np.tile(ref.twist(3.0, 0.1), (2, 1, 1))) == (0, 0) and refine_cpu._RefineMirrorMap.log == []  # an empty map
    depth, rgb = room_depth(W, H, K, torch.eye(4)), torch.full((H, W, 3), 100.0)
    render, alphas = torch.full((H, W), 0.01), torch.ones(H, W)
    alphas[:, 0] = 0.25
    m.insert_frame(depth, rgb, K, torch.eye(4), origin=0)
    for k in (1, 2, 5):
        m.insert_frame(depth, rgb, K, torch.eye(4), render, alphas, origin=k)
    poses = [np.eye(4, dtype=F32) for _ in range(3)]
    for k, p in enumerate(poses):
        p[0, 3] = 0.1 * k
    assert m.add_keyframe(depth, poses[0], origin=0) == 0 and m.add_keyframe(depth, poses[1], origin=2) == 1
    assert m.add_keyframe(depth, poses[2]) == 2  # no frame index on record
    with pytest.raises(ValueError, match="origin"):
        m.add_keyframe(depth, poses[2], origin=-1)
    n, ptr = m.n_live, m.means.data_ptr()
    means, colors, stamps, origins = m.points.clone(), m.point_colors.clone(), m.stamps.clone(), m.origins.clone()
    m._view_rows = n  # as after a select_view
    D = np.stack([np.eye(4), ref.twist(2.0, 0.05), ref.twist(4.0, 0.1)])  # frame 5 lies outside these
    got = m.correct(torch.from_numpy(D))
    call = refine_cpu._RefineMirrorMap.log[-1]
    assert call["call"] == "correct" and call["rows"] == n and np.array_equal(call["table"], ref.table_of(D))
    assert got == (2 * H, H) and call["moved"].tolist() == [False] * (W * H) + [True] * (2 * H) + [False] * H
    want = ref.correct(means.numpy(), origins[:n].numpy(), ref.table_of(D))["means"]
    assert np.array_equal(_bits(m.points.numpy()), _bits(want)) and m.means.data_ptr() == ptr and m.n_live == n
    assert not torch.equal(m.points[W * H:W * H + 2 * H], means[W * H:W * H + 2 * H])
    assert torch.equal(m.point_colors, colors) and torch.equal(m.stamps, stamps) and torch.equal(m.origins, origins)
    assert m._view_rows == -1
    with pytest.raises(RuntimeError, match="select_view"):
        m.view_violations(K, torch.eye(4), NEAR, 10.0)
    # the keyframes: the one of frame 0 keeps its bits, the one of frame 2 moves in float64, the third is left alone
    kf = m.keyframe_poses.numpy()
    assert np.array_equal(kf[0], poses[0]) and np.array_equal(kf[2], poses[2])
    assert np.array_equal(kf[1], (D[2] @ poses[1].astype(np.float64)).astype(F32)) and not np.array_equal(kf[1], poses[1])
    # all-identity transforms: nothing moves, the ballots stay valid
    m._view_rows, after = n, m.points.clone()
    assert m.correct(np.tile(np.eye(4), (6, 1, 1))) == (0, 0) and torch.equal(m.points, after) and m._view_rows == n
    assert np.array_equal(m.keyframe_poses.numpy(), kf)
    for bad in (np.eye(4), np.zeros((0, 4, 4)), np.zeros((2, 3, 4)), np.full((2, 4, 4), np.nan)):
        with pytest.raises(ValueError, match="transforms"):
            m.correct(bad)
    host = GaussianMap(W, H, MapConfig(origins=True), "cpu")
    host.n_live = 3
    with pytest.raises(AssertionError, match="no CPU path"):
        host.correct(D)


def test_loop_constraint_looks_at_the_prefix_only():
    """align_pose and score_poses are given rows_up_to(upto_frame) as their row count, and nothing else changes."""
    seen = []

    class _Map(_CorrectMirrorMap):
        def _align_launch(self, *args, n_rows=None):
            seen.append(("align", n_rows, self.n_live))
            w2c = args[2].numpy().astype(np.float64)
            return w2c[:3], w2c.astype(F32), 0, np.array([[2, 3, 5, 0]], np.int64), np.zeros((1, 6))  # FEW

        def _score_launch(self, depth, intr, w2c, near, n_rows=None):
            seen.append(("score", n_rows, len(w2c)))
            return np.arange(3 * len(w2c), dtype=np.int64).reshape(-1, 3)

    m = _Map(W, H, MapConfig(origins=True, capacity=W * H + 4 * H), "cpu")
    depth, rgb = room_depth(W, H, K, torch.eye(4)), torch.full((H, W, 3), 100.0)
    render, alphas = torch.full((H, W), 0.01), torch.ones(H, W)
    alphas[:, 0] = 0.25
    m.insert_frame(depth, rgb, K, torch.eye(4))
    for _ in range(3):
        m.insert_frame(depth, rgb, K, torch.eye(4), render, alphas)
    c = m.loop_constraint(depth, K, torch.eye(4), 1, NEAR, steps=1)
    assert isinstance(c, LoopConstraint) and isinstance(c.alignment, PoseAlignment) and c.alignment.status == "FEW"
    assert c.rows == m.rows_up_to(1) == W * H + H < m.n_live
    assert seen == [("align", c.rows, m.n_live), ("score", c.rows, 2)]
    assert c.scores.tolist() == [0, 1, 2] and c.aligned_scores.tolist() == [3, 4, 5]
    # no row up to that frame: nothing is launched, the alignment says FEW and the scores are zeros
    seen.clear()
    c = m.loop_constraint(depth, K, torch.eye(4), -1, NEAR)
    assert c.rows == 0 and seen == [] and c.alignment.status == "FEW" and not c.scores.any() and not c.aligned_scores.any()
    # the plain calls hand the launches no row count at all: mirrors written before the prefix keep working
    m.score_poses(depth, K, [torch.eye(4)], NEAR)
    m.align_pose(depth, K, torch.eye(4), NEAR)
    assert seen == [("score", None, 1), ("align", None, m.n_live)]
    for bad in (-1, m.n_live + 1, 1.5, True):
        with pytest.raises(ValueError, match="rows"):
            m.score_poses(depth, K, [torch.eye(4)], NEAR, rows=bad)
        with pytest.raises(ValueError, match="rows"):
            m.align_pose(depth, K, torch.eye(4), NEAR, rows=bad)


# ---- Localizer.close_loop around stand-ins --------------------------------------------------------------------------
def _localizer(config, monkeypatch, motion="hold"):
    import gsplatloc_amd.data.dataset as DS

    monkeypatch.setattr(DS, "compute_depth_gt", lambda pts, col, Ks, c2w, height, width: torch.zeros(height, width))
    base._Tracker.made = []
    refine_cpu._RefineMirrorMap.log = []
    return Localizer(K, W, H, TrackerConfig(max_steps=5), normalize=False, motion=motion, device="cpu",
                     tracker_factory=base._Tracker, mode="map", map_factory=_CorrectMirrorMap,
                     map_renderer=refine_cpu._Renderer(), map_config=config)


def test_the_localizer_writes_the_index_of_every_pose(sequence, monkeypatch):  # noqa: F811
    cfg = MapConfig(origins=True, reloc=True, keyframes=True, keyframe_rot_deg=0.05, keyframe_trans=0.001)
    loc = _localizer(cfg, monkeypatch)
    loc.reset(*sequence[0])
    for k in range(1, base.N_FRAMES):
        loc.track(sequence[k][0], sequence[k][1], gt_c2w=sequence[k][2])
    assert loc.map.origins[:loc.map.n_live].tolist() == [0] * (W * H) + [k for k in range(1, base.N_FRAMES) for _ in range(H)]
    assert loc.map._kf_origins[:loc.map.n_keyframes].tolist() == list(range(base.N_FRAMES))
    # a lost frame has a pose and no rows: the next frame's origin skips its index
    loc = _localizer(MapConfig(origins=True), monkeypatch)
    loc.reset(*sequence[0])
    loc._factory = base._LostTracker
    loc.tracker = None
    loc._tracker_N = -1
    assert loc.track(sequence[1][0], sequence[1][1]).lost
    loc._factory, loc._tracker_N = base._Tracker, -1
    loc.track(sequence[2][0], sequence[2][1], gt_c2w=sequence[2][2])
    assert loc.map.origins[:loc.map.n_live].tolist() == [0] * (W * H) + [2] * H and loc.trajectory.shape[0] == 3
    loc.reset(*sequence[0])  # reset() starts over at 0
    assert loc.map.origins[:loc.map.n_live].tolist() == [0] * (W * H)


def test_close_loop(sequence, monkeypatch):  # noqa: F811
    cfg = MapConfig(origins=True, reloc=True, keyframes=True, keyframe_rot_deg=0.05, keyframe_trans=0.001)
    loc = _localizer(cfg, monkeypatch, motion="constant_velocity")
    loc.reset(*sequence[0])
    for k in range(1, base.N_FRAMES):
        loc.track(sequence[k][0], sequence[k][1], gt_c2w=sequence[k][2])
    n, last = loc.map.n_live, base.N_FRAMES - 1
    old = loc.trajectory.double().numpy()
    means, origins = loc.map.points.clone(), loc.map.origins[:n].clone()
    kf = loc.map.keyframe_poses.numpy()
    target = ref.twist(1.5, 0.04) @ old[last]  # where the last frame really stood
    loc.map._view_rows = n
    refine_cpu._RefineMirrorMap.log = []
    out = loc.close_loop(1, last, torch.from_numpy(target).float())
    D = spread_correction(old, 1, last, target.astype(F32).astype(np.float64) @ np.linalg.inv(old[last]))
    # the poses are replaced: frames 0 and 1 bit for bit, the last one is the constraint
    new = loc.trajectory
    assert new.shape == (base.N_FRAMES, 4, 4) and new.dtype == torch.float32
    assert torch.equal(new[:2], torch.from_numpy(old[:2]).float())
    assert np.abs(new.double().numpy() - D @ old).max() <= 1e-6 and np.abs(new[last].double().numpy() - target).max() <= 1e-6
    # the map moved with them, by the mirror's rule on the table of those D
    call = [c for c in refine_cpu._RefineMirrorMap.log if c["call"] == "correct"]
    assert len(call) == 1 and np.abs(call[0]["table"] - ref.table_of(D)).max() <= 1e-6
    assert np.array_equal(call[0]["table"][:2], np.stack([EYE12] * 2))
    want = ref.correct(means.numpy(), origins.numpy(), call[0]["table"])
    assert np.array_equal(_bits(loc.map.points.numpy()), _bits(want["means"]))
    assert torch.equal(loc.map.points[:W * H + H], means[:W * H + H])  # frames 0 and 1
    assert isinstance(out, TrajectoryCorrection) and out.moved == (last - 1) * H == want["counters"][0]
    assert out.outside == 0 and out.frames == last - 1
    assert abs(out.max_rot_deg - 1.5) <= 1e-3 and abs(out.max_trans - np.linalg.norm(D[last, :3, 3])) <= 1e-6
    # the keyframe poses moved with their frames, the view ballots are stale
    kf2 = loc.map.keyframe_poses.numpy()
    assert np.array_equal(kf2[:2], kf[:2]) and np.abs(kf2 - (D @ kf.astype(np.float64))).max() <= 1e-6
    assert not np.array_equal(kf2[last], kf[last]) and loc.map._view_rows == -1
    # the motion model of the next frame reads the corrected poses
    r = loc.track(sequence[0][0], sequence[0][1])
    from gsplatloc_amd.localizer import predict_pose
    assert torch.equal(r.init_c2w, predict_pose(new[last - 1], new[last]))
    assert (loc.map.origins[loc.map.n_live - H:loc.map.n_live] == base.N_FRAMES).all()
    # poses given back as they are: nothing moves
    again = loc.trajectory
    before = loc.map.points.clone()
    out = loc.correct_trajectory(again)
    assert (out.moved, out.frames, out.max_trans, out.max_rot_deg) == (0, 0, 0.0, 0.0)
    assert torch.equal(loc.map.points, before) and torch.equal(loc.trajectory, again)
    # by="index", and what is refused
    assert loc.close_loop(0, 2, again[2], by="index").moved == 0  # the pose it already has
    with pytest.raises(ValueError):
        loc.correct_trajectory(again[:-1])
    with pytest.raises(ValueError):
        loc.close_loop(3, 3, again[3])
    with pytest.raises(ValueError):
        loc.close_loop(0, 99, again[3])
    with pytest.raises(ValueError):
        loc.close_loop(0, 3, torch.eye(3))
    with pytest.raises(ValueError):
        loc.close_loop(0, 3, torch.from_numpy(ref.twist(120.0, 0.0)) @ again[3].double())


def test_close_loop_needs_the_origins(sequence, monkeypatch):  # noqa: F811
    loc = _localizer(MapConfig(), monkeypatch)
    loc.reset(*sequence[0])
    loc.track(sequence[1][0], sequence[1][1], gt_c2w=sequence[1][2])
    assert loc.map.origins is None
    with pytest.raises(RuntimeError, match="origins"):
        loc.close_loop(0, 1, torch.eye(4))
    with pytest.raises(RuntimeError, match="origins"):
        loc.correct_trajectory(loc.trajectory)
    frame = Localizer(K, W, H, TrackerConfig(max_steps=5), normalize=False, device="cpu", tracker_factory=base._Tracker)
    with pytest.raises(RuntimeError, match="origins"):
        frame.close_loop(0, 1, torch.eye(4))
    fresh = _localizer(MapConfig(origins=True), monkeypatch)
    with pytest.raises(RuntimeError, match="reset"):
        fresh.correct_trajectory(torch.eye(4)[None])


def test_the_option_of_the_evaluation_driver_needs_the_map_mode(tmp_path, capsys):
    from gsplatloc_amd import eval as ev

    with pytest.raises(ValueError, match="map_origins"):
        ev.evaluate_room(None, 200, 3, sequential=True, map_origins=True)
    for extra in (["--map-origins"], ["--sequential", "--map-origins"]):
        with pytest.raises(SystemExit):
            ev.main(["--root", str(tmp_path)] + extra)
        assert "needs --map" in capsys.readouterr().err


# ---- the entry point ------------------------------------------------------------------------------------------------
BAD_ARG, OK = -1, 0
GOOD = dict(n_rows=1000, n_frames=3)
REFUSED = [("NULL means", dict(means=None)), ("NULL origins", dict(origins=None)), ("NULL table", dict(table=None)),
           ("NULL counters", dict(counters=None)), ("n_rows < 0", dict(n_rows=-1)), ("n_rows == 2^31", dict(n_rows=1 << 31)),
           ("n_rows == 2^40", dict(n_rows=1 << 40)), ("n_frames == 0", dict(n_frames=0)), ("n_frames < 0", dict(n_frames=-2)),
           ("no rows and no table", dict(n_rows=0, n_frames=0)), ("no rows and NULL means", dict(n_rows=0, means=None))]


def test_the_entry_point_rejects_bad_arguments_before_any_launch(repo_root):
    """Every row is refused on the host: the pointers are one dummy HOST buffer, a launch would give GSL_ERR_HIP or
    worse.  No rows at all is not an error, and launches nothing either."""
    lib = _lib.load_library()
    ret, params = prototypes(repo_root)["gsl_map_correct"]
    assert ret == "int" and [n for _, n in params] == ["means", "origins", "n_rows", "table", "n_frames", "counters",
                                                        "stream"]
    assert [t.replace(" ", "") for t, _ in params] == ["float*", "constint32_t*", "int64_t", "constfloat*", "int",
                                                        "int64_t*", "void*"]
    assert "gsl_map_correct" in _lib.exported_symbols()
    buf = ctypes.create_string_buffer(256)
    for what, over in REFUSED:
        named = dict(GOOD, **over)
        assert set(named) <= {n for _, n in params}, what
        assert lib.gsl_map_correct(*refine_cpu.refine_args(params, named, ctypes.addressof(buf))) == BAD_ARG, what
    assert lib.gsl_map_correct(*refine_cpu.refine_args(params, dict(GOOD, n_rows=0), ctypes.addressof(buf))) == OK
    assert not any(buf.raw)  # nothing wrote to the buffer, the counters included
    assert "map_correct.hip" in open(os.path.join(repo_root, "gsplatloc_amd", "csrc", "Makefile")).read()


# ---- the kernel's budget --------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_the_kernel_stays_in_registers():
    """No scratch, no LDS beyond the two words of the counts, no accumulation registers, eight waves per SIMD; 30
    vector registers is what the build gives ("Trajectory correction"): a change is worth a look."""
    res = _resources("map_correct.hip")
    assert len(res) == 1 and "k_map_correct" in list(res)[0], list(res)
    r = list(res.values())[0]
    assert r["ScratchSize"] == 0 and r["LDS"] <= 8 and r["AGPRs"] == 0 and r["Occupancy"] == 8 and r["VGPRs"] == 30, r
