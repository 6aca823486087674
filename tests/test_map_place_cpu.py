"""Keyframes and place recognition (csrc/map_place.hip, GaussianMap.describe / add_keyframe / match_place,
MapConfig.keyframes), the parts that need no GPU: the mirror of the two rules and of the ranking on hand-made cases,
MapConfig, the entry points against their prototypes and their argument checks, the keyframe decision and the ring, the
turn that a grid shift stands for, Localizer(mode="map") with ``keyframes`` around the stand-ins of
tests/test_map_score_cpu.py and a map whose device calls are the mirrors, the flags of the evaluation driver, and the
two kernels' resources.

The flow cases: the 32x24 box room of gsplatloc_amd.synthetic, seen from an off-centre position (from the centre the box
is symmetric, and two views half a turn apart are the same image).  Frame 0 -- keyframe 0 -- is taken at P0, 120 degrees
about y.  A second frame at FAR, 40 degrees back, is placed by a stand-in that answers its ground truth; it is accepted
and becomes keyframe 1.  The kidnapped frame is taken at KID = place_base(P0, 1, 0): P0 turned by the one-cell yaw (7.1
degrees), so that candidate 0 of the place grid is its pose.  From now on the stand-in answers its start pose.  The hold
start, FAR, is rejected, and so is the winner of the grid around it (two steps of 2 degrees); with the mirrors keyframe
0 matches best under the shift (1, 0) -- sum / common 115 against 521 for keyframe 1 -- and candidate 0 wins the place
grid with agree - front 656 against 655."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from gsplatloc_amd import _lib, mapping
from gsplatloc_amd.localizer import Localizer, LocalizeResult, _step, place_base, reloc_candidates
from gsplatloc_amd.mapping import GaussianMap, MapConfig, rank_places
from gsplatloc_amd.my_gsplat import TrackerConfig
from gsplatloc_amd.my_gsplat.trainer import TrackResult
from gsplatloc_amd.synthetic import replica_intrinsics, room_depth
from tests import map_place_ref as ref
from tests import map_score_ref as score_ref
from tests import test_map_cpu as base
from tests import test_map_score_cpu as score_cpu
from tests.pose_ref import axis_angle
from tests.test_abi import prototypes
from tests.test_kernel_resources import HIPCC, _resources

F32 = np.float32
NAN, INF = float("nan"), float("inf")


# ---- the mirror of the descriptor -----------------------------------------------------------------------------------
def test_descriptor_one_pixel_per_cell():
    """16 x 12: every pixel is its own cell; dyadic depths make d * 1024 exact, a cell's value is its pixel's q."""
    d = (np.arange(192, dtype=F32).reshape(12, 16) + 1) / F32(64.0)  # 1/64 .. 3 m
    got = ref.describe(d)
    assert got.dtype == np.int32 and got.shape == (192,)
    assert got.tolist() == [16 * (k + 1) for k in range(192)]
    d[3, 5], d[0, 0], d[11, 15] = 0.0, NAN, INF  # a cell of one pixel without depth: 0 of 1, invalid
    got = ref.describe(d)
    assert got[3 * 16 + 5] == got[0] == got[191] == -1 and (got >= 0).sum() == 189


def test_descriptor_cells_of_an_uneven_image():
    """33 x 17: the cell of every pixel is ((u * 16) // W, (v * 12) // H); cells are 2 or 3 columns by 1 or 2 lines."""
    W, H = 33, 17
    d = np.zeros((H, W), F32)
    members = {}
    for v in range(H):
        for u in range(W):
            members.setdefault(ref.cell_of(u, v, W, H), []).append((u, v))
    assert sorted(members) == [(i, j) for i in range(16) for j in range(12)]
    assert {len(m) for m in members.values()} == {2, 3, 4, 6}
    assert ref.cell_of(0, 0, W, H) == (0, 0) and ref.cell_of(32, 16, W, H) == (15, 11) and ref.cell_of(2, 1, W, H) == (0, 0)
    assert ref.cell_of(3, 2, W, H) == (1, 1)  # 48 // 33, 24 // 17
    # one cell at a time: light exactly its pixels, and only its entry is valid and holds their floored mean
    for (ci, cj), pixels in members.items():
        d[:] = 0.0
        for n, (u, v) in enumerate(pixels):
            d[v, u] = 1.0 + n / 1024.0  # q = 1024 + n
        got = ref.describe(d)
        want = (1024 * len(pixels) + sum(range(len(pixels)))) // len(pixels)
        assert got[cj * 16 + ci] == want and (got >= 0).sum() == 1, (ci, cj)


def test_descriptor_half_of_a_cell_is_enough_and_one_less_is_not():
    """32 x 24, cells of 2 x 2: 2 valid pixels of 4 are valid, 1 is not.  48 x 36, cells of 3 x 3 = 9 pixels: 5 valid
    are (2 * 5 >= 9), 4 are not."""
    d = np.zeros((24, 32), F32)
    d[0, 0] = d[1, 1] = 2.0  # cell (0, 0): 2 of 4
    d[0, 2] = 2.0  # cell (1, 0): 1 of 4
    got = ref.describe(d)
    assert got[0] == 2048 and got[1] == -1 and (got >= 0).sum() == 1
    d = np.zeros((36, 48), F32)
    d[0, 0:3], d[1, 0:2] = 1.0, 1.0  # cell (0, 0): 5 of 9
    d[0, 3:6], d[1, 3] = 1.0, 1.0  # cell (1, 0): 4 of 9
    got = ref.describe(d)
    assert got[0] == 1024 and got[1] == -1 and (got >= 0).sum() == 1


def test_descriptor_pixels_that_do_not_count():
    """NaN, inf, -inf, 0, -0 and negative depths are left out of the sum AND of the count; a depth above 63 m clamps."""
    d = np.full((24, 32), 1.0, F32)  # cells of 2 x 2
    bad = [NAN, INF, -INF, 0.0, -0.0, -2.0]
    for k, b in enumerate(bad):  # cell k: one bad pixel, 3 of 4 count, the mean is still 1 m
        d[0, 2 * k] = b
    d[2, 0:2], d[3, 0] = NAN, -1.0  # cell (0, 1): 1 of 4
    d[2, 2], d[3, 2] = 1000.0, 63.5  # cell (1, 1): two clamped pixels, 64 512 each, and two at 1 m
    d[2, 4] = 63.0  # cell (2, 1): exactly at the clamp
    got = ref.describe(d)
    assert got[:6].tolist() == [1024] * 6 and got[16] == -1
    assert got[17] == (2 * 64512 + 2 * 1024) // 4 and got[18] == (64512 + 3 * 1024) // 4 and ref.Q_MAX == 64512
    counts, q = ref.quantise(np.array([[NAN, INF, -INF, 0.0, -0.0, -2.0, 1e30, 63.0, 1.0]], F32))
    assert counts.tolist() == [[False] * 6 + [True] * 3] and q.tolist() == [[0] * 6 + [64512, 64512, 1024]]


def test_descriptor_rounds_half_to_even_and_floors_the_mean():
    """d * 1024 ending in .5 goes to the even neighbour (rintf), and sum / count is floored."""
    halves = np.array([[0.5 / 1024, 1.5 / 1024, 2.5 / 1024, 3.5 / 1024, 1000.5 / 1024, 1001.5 / 1024]], F32)
    assert (halves * F32(1024.0)).tolist() == [[0.5, 1.5, 2.5, 3.5, 1000.5, 1001.5]]  # exact products
    assert ref.quantise(halves)[1].tolist() == [[0, 2, 2, 4, 1000, 1002]]
    d = np.zeros((24, 32), F32)
    d[0, 0], d[0, 1], d[1, 0] = 1.0, 1.0, 1.0 + 2.0 / 1024  # 1024 + 1024 + 1026 = 3074, / 3 = 1024.67
    assert ref.describe(d)[0] == 1024
    d[1, 1] = 0.5 / 1024  # counts (d > 0), and its q is 0
    assert ref.describe(d)[0] == 3074 // 4


# ---- the mirror of the match and the ranking ------------------------------------------------------------------------
def test_match_shifts_worked_out_by_hand():
    assert ref.SHIFTS[0] == (-2, -1) and ref.SHIFTS[7] == (0, 0) and ref.SHIFTS[14] == (2, 1) and len(ref.SHIFTS) == 15
    assert ref.SHIFTS == [(sx, sy) for sy in (-1, 0, 1) for sx in (-2, -1, 0, 1, 2)] == list(mapping.PLACE_SHIFTS)
    table = (np.arange(192, dtype=np.int32).reshape(12, 16) * 10).copy()  # t[j][i] = 10 (16 j + i)
    query = np.full((12, 16), 7, np.int32)
    table[0, 0], query[11, 15], query[5, 5] = -1, -1, -1
    got = ref.match(query.reshape(-1), table.reshape(1, -1))
    assert got.shape == (1, 15, 2) and got.dtype == np.int64
    # (0, 0): all 192 cells but table (0, 0), query (15, 11) and query (5, 5); |7 - 10 c| = 10 c - 7 for c >= 1
    cells = [c for c in range(192) if c not in (0, 191, 5 * 16 + 5)]
    assert got[0, 7].tolist() == [189, sum(10 * c - 7 for c in cells)]
    # (2, 1): table cells i <= 13, j <= 10 meet query (i + 2, j + 1); table (0, 0) is invalid, query (15, 11) meets
    # table (13, 10), query (5, 5) meets table (3, 4)
    cells = [16 * j + i for j in range(11) for i in range(14) if (i, j) not in ((0, 0), (13, 10), (3, 4))]
    assert got[0, 14].tolist() == [14 * 11 - 3, sum(10 * c - 7 for c in cells)]
    # (-2, -1): table cells i >= 2, j >= 1 meet query (i - 2, j - 1); query (5, 5) meets table (7, 6); query (15, 11)
    # and table (0, 0) meet nothing
    cells = [16 * j + i for j in range(1, 12) for i in range(2, 16) if (i, j) != (7, 6)]
    assert got[0, 0].tolist() == [14 * 11 - 1, sum(10 * c - 7 for c in cells)]
    # the direction: what the keyframe holds at (i, j) the query holds at (i + sx, j + sy)
    t = np.full((12, 16), -1, np.int32)
    q = t.copy()
    t[4, 6], q[5, 8] = 500, 500
    got = ref.match(q.reshape(-1), np.stack([t.reshape(-1)]))[0]
    assert [tuple(r) for r in got.tolist()] == [(1, 0) if s == (2, 1) else (0, 0) for s in ref.SHIFTS]


def _result(entries, n=1):
    """[n,15,2] (common, sum) with the named (slot, shift index) entries set and nothing else admissible."""
    r = np.zeros((n, 15, 2), np.int64)
    for (slot, s), (total, common) in entries.items():
        r[slot, s] = common, total
    return r


@pytest.mark.parametrize("rank", [ref.rank, rank_places], ids=["mirror", "rank_places"])
def test_ranking_and_every_tie_break(rank):
    # the smallest sum / common wins, compared exactly: 1000001 / 100 against 1000000 / 100, and 2 / 3 against 4 / 6
    r = _result({(0, 7): (1000001, 100), (0, 3): (1000000, 100)})
    assert rank(r, 48) == [(0, 1, -1, 1000000, 100)]
    big = 192 * 64512
    assert rank(_result({(0, 2): (big, 191), (0, 7): (big + 1, 191)}), 48) == [(0, 0, -1, big, 191)]
    # a shift with fewer common cells than asked for does not count, however well it matches
    r = _result({(0, 7): (0, 47), (0, 0): (5000, 48)})
    assert rank(r, 48) == [(0, -2, -1, 5000, 48)] and rank(r, 47) == [(0, 0, 0, 0, 47)] and rank(r, 49) == []
    # equal fractions: the smaller |sx| + |sy| -- (0, 0) over (1, 0) over (2, 1)
    r = _result({(0, 14): (200, 100), (0, 8): (400, 200), (0, 7): (300, 150)})
    assert rank(r, 48) == [(0, 0, 0, 300, 150)]
    r = _result({(0, 14): (200, 100), (0, 8): (400, 200)})
    assert rank(r, 48) == [(0, 1, 0, 400, 200)]
    # equal fractions, equal |sx| + |sy|: the earlier shift -- (0, -1) is shift 2, (-1, 0) is 6, (1, 0) is 8, (0, 1) is 12
    r = _result({(0, 12): (100, 50), (0, 8): (100, 50), (0, 6): (200, 100), (0, 2): (300, 150)})
    assert rank(r, 48) == [(0, 0, -1, 300, 150)]
    r = _result({(0, 12): (100, 50), (0, 8): (100, 50), (0, 6): (200, 100)})
    assert rank(r, 48) == [(0, -1, 0, 200, 100)]
    # between keyframes: the fraction, then |sx| + |sy|, then the shift, then the slot; no admissible shift: left out
    r = _result({(0, 7): (300, 100), (1, 8): (200, 100), (2, 7): (200, 100), (3, 6): (400, 200), (5, 7): (100, 50),
                 (6, 0): (1, 47)}, n=7)
    assert rank(r, 48) == [(2, 0, 0, 200, 100), (5, 0, 0, 100, 50), (3, -1, 0, 400, 200), (1, 1, 0, 200, 100),
                           (0, 0, 0, 300, 100)]
    assert rank(_result({}, n=3), 48) == []


# ---- MapConfig ------------------------------------------------------------------------------------------------------
def test_map_config_validation():
    c = MapConfig()
    assert (c.keyframes, c.keyframe_max, c.keyframe_rot_deg, c.keyframe_trans, c.place_top, c.place_min_common) == (
        False, 256, 6.0, 0.15, 2, 48)
    ok = MapConfig(reloc=True, keyframes=True, keyframe_max=1, keyframe_rot_deg=0.5, keyframe_trans=1e-3, place_top=1,
                   place_min_common=192)
    assert ok.keyframes and MapConfig(reloc=True, keyframes=True, keyframe_max=256, place_min_common=1).keyframe_max == 256
    bad = dict(keyframes=[1, "yes", None, 0.5],
               keyframe_max=[0, 257, -1, 1.0, True, "8", None],
               keyframe_rot_deg=[0.0, -1.0, INF, NAN, True, "6", None],
               keyframe_trans=[0.0, -0.05, INF, NAN, False, "0.1", None],
               place_top=[0, -1, 1.0, True, "2", None, 3, 64],
               place_min_common=[0, 193, -4, 48.0, True, "48", None])
    for field, values in bad.items():
        for v in values:
            with pytest.raises(ValueError, match=field):
                MapConfig(reloc=True, **{field: v})
    # keyframes without reloc
    with pytest.raises(ValueError, match="keyframes.*reloc"):
        MapConfig(keyframes=True)
    # place_top against the 64 poses of one scoring call: 1 + 12 levels poses per base
    assert MapConfig(reloc_levels=2, place_top=2).place_top == 2 and MapConfig(reloc_levels=1, place_top=4).place_top == 4
    for levels, top in ((2, 3), (1, 5)):
        with pytest.raises(ValueError, match="place_top.*64"):
            MapConfig(reloc_levels=levels, place_top=top)


# ---- the entry points -----------------------------------------------------------------------------------------------
DESCRIBE, MATCH = "gsl_map_place_describe", "gsl_map_place_match"
GOOD = {DESCRIBE: dict(width=160, height=120), MATCH: dict(n_keyframes=3)}
REFUSED = {
    DESCRIBE: [("NULL depth", dict(depth=None)), ("NULL desc", dict(desc=None)), ("width 15", dict(width=15)),
               ("height 11", dict(height=11)), ("width 0", dict(width=0)), ("height < 0", dict(height=-120)),
               ("a cell of 65 537 pixels", dict(width=16 * 65537, height=12)),
               ("a cell of 257 x 256", dict(width=16 * 257, height=12 * 256)),
               ("the largest cell of an uneven image", dict(width=16 * 256 + 1, height=12 * 256)),
               ("2^31 - 1 squared", dict(width=2 ** 31 - 1, height=2 ** 31 - 1))],
    MATCH: [("NULL query", dict(query=None)), ("NULL table", dict(table=None)), ("NULL out", dict(out=None)),
            ("no keyframe", dict(n_keyframes=0)), ("n_keyframes < 0", dict(n_keyframes=-1)),
            ("257 keyframes", dict(n_keyframes=257))],
}


def test_header_binding_and_definitions_agree(repo_root):
    protos = prototypes(repo_root)
    assert protos[DESCRIBE] == ("int", [("const float*", "depth"), ("int", "width"), ("int", "height"),
                                        ("int32_t*", "desc"), ("void*", "stream")])
    assert protos[MATCH] == ("int", [("const int32_t*", "query"), ("const int32_t*", "table"), ("int", "n_keyframes"),
                                     ("int32_t*", "out"), ("void*", "stream")])
    assert protos["gsl_map_place_cells"] == ("int", [])
    src = open(os.path.join(repo_root, "gsplatloc_amd", "csrc", "map_place.hip")).read()
    for fn in (DESCRIBE, MATCH):
        assert len(_lib._SIGNATURES[fn][1]) == len(protos[fn][1])
        m = re.search(r'extern "C" int %s\((.*?)\)\s*\{' % fn, src, flags=re.S)
        assert m, fn
        defined = [re.fullmatch(r"\s*(.*?)\s*(\w+)\s*", p, flags=re.S).groups() for p in m.group(1).split(",")]
        assert [(" ".join(t.split()), n) for t, n in defined] == protos[fn][1]
    header = open(os.path.join(repo_root, "include", "gsloc_hip.h")).read()
    gw, gh, most = (int(re.search(r"#define GSL_MAP_PLACE_%s (\d+)" % n, header).group(1))
                    for n in ("GW", "GH", "MAX_KEYFRAMES"))
    assert (gw, gh) == (16, 12) == (ref.GW, ref.GH) == (mapping.PLACE_GW, mapping.PLACE_GH)
    assert gw * gh == 192 == ref.CELLS == mapping.PLACE_CELLS == _lib.load_library().gsl_map_place_cells()
    assert most == 256 == mapping.PLACE_MAX_KEYFRAMES
    assert "map_place.hip" in open(os.path.join(repo_root, "gsplatloc_amd", "csrc", "Makefile")).read()


@pytest.mark.parametrize("fn", [DESCRIBE, MATCH])
def test_entry_points_reject_bad_arguments_before_any_launch(fn, repo_root, monkeypatch):
    """Every row is refused on the host: the pointers are one dummy HOST buffer, a launch would give GSL_ERR_HIP or
    worse.  The caller is that of tests/test_map_score_cpu.py, pointed at these entry points."""
    monkeypatch.setattr(score_cpu, "FN", fn)
    lib = _lib.load_library()
    params = prototypes(repo_root)[fn][1]
    buf = ctypes.create_string_buffer(b"\x7f" * 1024, 1024)
    pointers = {n: ctypes.addressof(buf) for t, n in params if "*" in t}
    for what, over in REFUSED[fn]:
        named = dict(GOOD[fn], **over)
        assert set(named) <= {n for _, n in params}, what
        assert score_cpu.call_with(lib, params, named, pointers) == score_cpu.BAD_ARG, (fn, what)
    assert buf.raw == b"\x7f" * 1024  # nothing wrote to the buffer


# ---- GaussianMap: keyframes around the mirrors ------------------------------------------------------------------------
W, H = base.W, base.H
K = replica_intrinsics(W, H)
FX, FY = float(K[0, 0]), float(K[1, 1])
CFG_NEAR = TrackerConfig().gs.near_plane
STEP = 0.4  # metres: the translation step of the flow cases' grids
POSITION = (0.6, 0.1, 0.8)  # off the room's centre


class _PlaceMirrorMap(score_cpu._ScoreMirrorMap):
    """GaussianMap whose device calls are the numpy mirrors; the calls go to the log of _ScoreMirrorMap."""

    def _describe_launch(self, depth, desc):
        desc.copy_(torch.from_numpy(ref.describe(depth.numpy())))
        score_cpu._ScoreMirrorMap.log.append(dict(call="describe", depth=depth.clone()))

    def _match_launch(self, query, table, n):
        result = ref.match(query.numpy(), table[:n].numpy())
        score_cpu._ScoreMirrorMap.log.append(dict(call="match", query=query.clone(), n=n, result=result))
        return result


def _log():
    return score_cpu._ScoreMirrorMap.log


def _calls(*kinds):
    return [c["call"] for c in _log() if not kinds or c["call"] in kinds]


def _pose(yaw_deg, position=POSITION):
    c2w = torch.eye(4)
    c2w[:3, :3] = axis_angle((0.0, 1.0, 0.0), yaw_deg).float()
    c2w[:3, 3] = torch.tensor(position)
    return c2w


def _turned(c2w, axis, deg, metres=0.0, along=0):
    """c2w turned by deg about its own axis, then moved by metres along its own axis ``along`` (float32)."""
    return (c2w.double() @ _step(axis, rot_deg=deg) @ _step(along, trans=metres)).float()


def _frame_at(c2w, seed=0):
    rgb = torch.randint(0, 255, (H, W, 3), generator=torch.Generator().manual_seed(seed)).float()
    return room_depth(W, H, K, c2w), rgb


def _map(**cfg):
    score_cpu._ScoreMirrorMap.log = []
    return _PlaceMirrorMap(W, H, MapConfig(reloc=True, keyframes=True, **cfg), "cpu")


def test_add_keyframe_decides_on_the_host_from_the_stored_poses():
    m = _map()  # 6 degrees, 0.15 m
    depth = _frame_at(_pose(0.0))[0]
    assert m.n_keyframes == 0 and m.keyframe_poses.shape == (0, 4, 4) and m._place is None
    assert m.add_keyframe(depth, _pose(0.0)) == 0 and m.n_keyframes == 1  # the first frame always
    # within both thresholds of a stored one: none, and nothing is launched
    n_calls = len(_log())
    for near in (_pose(0.0), _turned(_pose(0.0), 1, 5.9), _turned(_pose(0.0), 0, -5.9, 0.149, 2),
                 _turned(_pose(0.0), 2, 3.0, -0.1, 0)):
        assert m.add_keyframe(depth, near) is None
    assert m.n_keyframes == 1 and len(_log()) == n_calls
    # beyond either: one
    assert m.add_keyframe(depth, _turned(_pose(0.0), 1, 6.1)) == 1  # the angle alone
    assert m.add_keyframe(depth, _turned(_pose(0.0), 1, 0.0, 0.151, 0)) == 2  # the distance alone
    # ... from EVERY stored pose: 6.1 degrees from keyframe 0 but 0 from keyframe 1 is none
    assert m.add_keyframe(depth, _turned(_pose(0.0), 1, 6.1)) is None
    assert m.add_keyframe(depth, _turned(_pose(0.0), 1, 12.3)) == 3 and m.n_keyframes == 4
    assert _calls() == ["describe"] * 4
    poses = m.keyframe_poses
    assert poses.dtype == torch.float32 and poses.device.type == "cpu" and torch.equal(poses[0], _pose(0.0))
    assert torch.equal(poses[3], _turned(_pose(0.0), 1, 12.3))
    # the descriptor went straight into the slot's row of the table; rows never used stay invalid
    assert np.array_equal(m._place["table"][2].numpy(), ref.describe(depth.numpy()))
    assert m._place["table"].shape == (256, 192) and int((m._place["table"][4:] != -1).sum()) == 0
    m.clear()
    assert m.n_keyframes == 0 and m.match_place(depth) == [] and m.add_keyframe(depth, _pose(0.0)) == 0
    with pytest.raises(ValueError, match=r"\(4, 4\)"):
        m.add_keyframe(depth, torch.eye(3))
    with pytest.raises(ValueError, match="depth"):
        m.add_keyframe(torch.ones(H, W + 1), _pose(50.0))
    off = _PlaceMirrorMap(W, H, MapConfig(), "cpu")
    for call in (lambda: off.add_keyframe(depth, _pose(0.0)), lambda: off.match_place(depth)):
        with pytest.raises(RuntimeError, match="keyframes"):
            call()
    host = GaussianMap(W, H, MapConfig(reloc=True, keyframes=True), "cpu")
    for call in (lambda: host.describe(depth), lambda: host.add_keyframe(depth, _pose(0.0))):
        with pytest.raises(AssertionError, match="no CPU path"):
            call()


def test_the_ring_overwrites_the_oldest_keyframe():
    m = _map(keyframe_max=3)
    frames = [(_frame_at(_pose(40.0 * k))[0], _pose(40.0 * k)) for k in range(5)]
    assert [m.add_keyframe(*f) for f in frames[:3]] == [0, 1, 2] and m.n_keyframes == 3
    assert m.add_keyframe(*frames[3]) == 0 and m.n_keyframes == 3  # keyframe_max + 1: slot 0 again
    assert torch.equal(m.keyframe_poses[0], frames[3][1]) and torch.equal(m.keyframe_poses[1], frames[1][1])
    assert np.array_equal(m._place["table"][0].numpy(), ref.describe(frames[3][0].numpy()))
    # the pose that was overwritten no longer holds a new frame off: frame 0's pose is a keyframe again, in slot 1
    assert m.add_keyframe(*frames[0]) == 1 and m.add_keyframe(*frames[0]) is None
    assert m._place["table"].shape == (3, 192)


def test_describe_and_match_place_hand_the_mirrors_what_the_kernels_get():
    m = _map(keyframe_rot_deg=20.0)
    views = [_frame_at(_pose(60.0 * k))[0] for k in range(3)]
    for k, d in enumerate(views):
        assert m.add_keyframe(d, _pose(60.0 * k)) == k
    got = m.describe(views[1])
    assert got.dtype == torch.int32 and got.shape == (192,) and np.array_equal(got.numpy(), ref.describe(views[1].numpy()))
    score_cpu._ScoreMirrorMap.log = []
    ranked = m.match_place(views[1])
    assert _calls() == ["describe", "match"]  # one launch each, one read-back
    call = _log()[1]
    assert call["n"] == 3 and np.array_equal(call["query"].numpy(), ref.describe(views[1].numpy()))
    assert ranked == ref.rank(call["result"], 48) and ranked[0] == (1, 0, 0, 0, 192) and len(ranked) == 3
    # place_min_common: with every cell asked for only the unshifted comparison is admissible
    strict = _map(keyframe_rot_deg=20.0, place_min_common=192)
    strict.add_keyframe(views[0], _pose(0.0))
    assert [r[1:3] for r in strict.match_place(views[1])] == [(0, 0)]
    with pytest.raises(ValueError, match="depth"):
        m.match_place(torch.ones(H + 1, W))


# ---- the turn that a shift stands for -------------------------------------------------------------------------------
def _angle_between(a, b):
    R = a[:3, :3].double().T @ b[:3, :3].double()
    return float(np.degrees(np.arccos(np.clip((float(R.trace()) - 1.0) / 2.0, -1.0, 1.0))))


@pytest.mark.parametrize("size", [(32, 24), (160, 120)])
def test_a_turned_camera_matches_under_the_shift_that_place_base_undoes(size, capsys):
    """One room frame at P is the only keyframe; queries at P @ R_y(-a) for sx in -2 .. 2 and at P @ R_x(+b) for sy in
    -1 .. 1, a and b the angles of sx and sy cells.  The best shift is (sx, 0), respectively (0, sy), and the base
    composed from it is nearer in rotation to the query's pose than P is (here: it is the query's pose).  This holds the
    sign of the two turns of place_base.  P is a pose at which the bare box gives the match enough to go by: over 3
    positions x 12 yaws the mirror finds a one-cell yaw exactly in 54 of 72 queries and within a cell in 71, a two-cell
    yaw exactly in 21 and within a cell in 67 (the descriptor is of z-depth, which a turn changes; NOTES.md, "Place
    recognition").  Printed: sum / common of the best and of the next shift."""
    w, h = size
    Kc = replica_intrinsics(w, h)
    fx, fy = float(Kc[0, 0]), float(Kc[1, 1])
    P = _pose(120.0)
    table = ref.describe(room_depth(w, h, Kc, P).numpy())[None]
    lines = []
    for sx, sy in [(s, 0) for s in range(-2, 3)] + [(0, -1), (0, 1)]:
        a, b = np.degrees(np.arctan(sx * (w / 16.0) / fx)), np.degrees(np.arctan(sy * (h / 12.0) / fy))
        Q = (P.double() @ _step(1, rot_deg=-a) @ _step(0, rot_deg=b)).float()
        result = ref.match(ref.describe(room_depth(w, h, Kc, Q).numpy()), table)
        ranked = ref.rank(result, 48)
        per_cell = sorted((t / c, ref.SHIFTS[s]) for s, (c, t) in enumerate(result[0].tolist()) if c >= 48)
        lines.append(f"({sx}, {sy}): best {ranked[0][1:]} sum / common {per_cell[0][0]:.1f}, next {per_cell[1][1]} "
                     f"{per_cell[1][0]:.1f}")
        assert ranked[0][:3] == (0, sx, sy), (size, sx, sy, ranked)
        found = place_base(P, ranked[0][1], ranked[0][2], w, h, fx, fy)
        assert _angle_between(found, Q) < 0.05 and (sx == sy == 0 or _angle_between(P, Q) > 5.0)
        assert torch.equal(found[:3, 3], P[:3, 3])
    with capsys.disabled():
        print(f"[place] turn from a shift at {w}x{h}: " + "; ".join(lines))
    assert torch.equal(place_base(P, 0, 0, w, h, fx, fy), P)  # no shift: bit for bit


# ---- Localizer(mode="map", keyframes) around the mirrors ------------------------------------------------------------
class _Tracker(score_cpu._StartTracker):
    """The stand-in of tests/test_map_score_cpu.py, run() answers its start pose; with ``truth`` set it answers the
    reference pose it was loaded with (the frame's ground truth) instead, which is how the flow cases grow a map."""
    truth = False

    def run(self):
        if not type(self).truth:
            return super().run()
        gt = self.loads[-1]["src_c2w"]
        return TrackResult(best_loss=0.25, steps=12, final_c2w=gt.clone(), best_c2w=gt.clone(), best_step=7)


class _Renderer(base._Renderer):
    """The stand-in renderer of tests/test_map_cpu.py: the first image column is new in every frame."""


def _localizer(monkeypatch, first, **cfg):
    import gsplatloc_amd.data.dataset as DS

    monkeypatch.setattr(DS, "compute_depth_gt", lambda pts, col, Ks, c2w, height, width: torch.zeros(height, width))
    _Tracker.made = base._Tracker.made = []
    _Tracker.truth = False
    loc = Localizer(K, W, H, TrackerConfig(max_steps=5), normalize=False, motion="hold", device="cpu",
                    tracker_factory=_Tracker, mode="map", map_factory=_PlaceMirrorMap, map_renderer=_Renderer(),
                    map_config=MapConfig(reloc=True, reloc_trans=STEP, **cfg))
    score_cpu._ScoreMirrorMap.log = []
    loc.reset(*_frame_at(first), first)
    return loc


P0, FAR = _pose(120.0), _pose(80.0)
KID = place_base(P0, 1, 0, W, H, FX, FY)
PER_BASE = 1 + 12 * 2  # poses of a grid per base, at the default reloc_levels


def _grown(monkeypatch, **cfg):
    """Frame 0 at P0 (keyframe 0), then a frame at FAR that the stand-in places with its ground truth; the log starts
    after it."""
    loc = _localizer(monkeypatch, P0, **cfg)
    _Tracker.truth = True
    r = loc.track(*_frame_at(FAR, 1), gt_c2w=FAR)
    _Tracker.truth = False
    assert torch.equal(loc.trajectory[-1], FAR)
    score_cpu._ScoreMirrorMap.log = []
    return loc, r


def _sizes():
    """Poses per score call of the log."""
    return [len(c["w2c"]) for c in _log() if c["call"] == "score"]


def _w2cs(poses):
    return np.stack([score_ref.w2c_of(p.numpy()) for p in poses])


def test_reset_keeps_the_first_frame_and_an_accepted_frame_is_offered(monkeypatch):
    loc = _localizer(monkeypatch, P0, keyframes=True)
    assert _calls() == ["insert", "describe"] and loc.map.n_keyframes == 1  # after the insertion
    assert torch.equal(loc.map.keyframe_poses[0], P0)
    assert np.array_equal(loc.map._place["table"][0].numpy(), ref.describe(_frame_at(P0)[0].numpy()))
    _Tracker.truth = True
    r = loc.track(*_frame_at(FAR, 1), gt_c2w=FAR)
    # accepted at once: nothing is matched; its insertion comes before its descriptor
    assert _calls() == ["insert", "describe", "score", "insert", "describe"]
    assert (r.lost, r.relocalised, r.recognised, r.keyframe) == (False, False, -1, 1) and loc.map.n_keyframes == 2
    assert torch.equal(loc.map.keyframe_poses[1], FAR)
    # a frame within 6 degrees and 15 cm of a keyframe is none, and launches nothing
    near = _turned(FAR, 1, 3.0)
    r = loc.track(*_frame_at(near, 2), gt_c2w=near)
    assert _calls()[5:] == ["score", "insert"] and (r.lost, r.keyframe, r.recognised) == (False, None, -1)
    loc.reset(*_frame_at(FAR), FAR)  # forgets the keyframes with the map
    assert loc.map.n_keyframes == 1 and torch.equal(loc.map.keyframe_poses[0], FAR)


def test_a_frame_the_grid_leaves_lost_is_recognised(monkeypatch, capsys):
    loc, grown = _grown(monkeypatch, keyframes=True)
    assert (grown.lost, grown.keyframe, loc.map.n_keyframes) == (False, 1, 2)
    depth, rgb = _frame_at(KID, 2)
    rows, n0 = loc.map.points.numpy().copy(), loc.map.n_live
    cfg = loc.map.cfg
    # what the mirrors say on host copies, before the frame is tracked
    grid1 = reloc_candidates([FAR], cfg.reloc_rot_deg, cfg.reloc_trans, cfg.reloc_levels)
    intr = (FX, FY, float(K[0, 2]), float(K[1, 2]))
    score = lambda poses: score_ref.score(rows, _w2cs(poses), intr, depth.numpy(), F32(loc.map.keep),  # noqa: E731
                                          F32(loc.map.beyond), CFG_NEAR)
    s1 = score(list(grid1))
    m1 = (s1[:, 1] - s1[:, 2]).tolist()
    w1 = m1.index(max(m1))
    share = lambda c: c[1] / max(c[1] + c[2], 1)  # noqa: E731
    assert share(s1[0]) < cfg.reloc_min_agree and w1 != 0 and share(s1[w1]) < cfg.reloc_min_agree  # rejected twice
    table = np.stack([ref.describe(_frame_at(p, k)[0].numpy()) for k, p in enumerate((P0, FAR))])
    ranked = ref.rank(ref.match(ref.describe(depth.numpy()), table), cfg.place_min_common)
    assert ranked[0][:3] == (0, 1, 0) and ranked[1][0] == 1
    bases = [place_base(p, r[1], r[2], W, H, FX, FY) for p, r in zip((P0, FAR), ranked)]
    assert torch.equal(bases[0], KID)
    grid2 = reloc_candidates(bases, cfg.reloc_rot_deg, cfg.reloc_trans, cfg.reloc_levels)
    s2 = score(list(grid2))
    m2 = (s2[:, 1] - s2[:, 2]).tolist()
    assert grid2.shape[0] == 2 * PER_BASE and m2.index(max(m2)) == 0 and s2[0, 2] == 0
    with capsys.disabled():
        print(f"[place] flow at {W}x{H}: start {s1[0].tolist()}, grid winner {w1} {s1[w1].tolist()}; match "
              f"{[(r[0], r[1], r[2], round(r[3] / r[4], 1)) for r in ranked]}; place grid winner 0 {s2[0].tolist()}, "
              f"runner-up agree - front {sorted(m2)[-2]}")
    r = loc.track(depth, rgb, gt_c2w=KID)
    # score, grid score, second score, match, grid score, third score, insert; the descriptors around them
    assert _calls() == ["score", "score", "score", "describe", "match", "score", "score", "insert", "describe"]
    assert _sizes() == [1, PER_BASE, 1, 2 * PER_BASE, 1]
    scores = [c for c in _log() if c["call"] == "score"]
    assert np.array_equal(scores[1]["w2c"], _w2cs(grid1)) and np.array_equal(scores[1]["counts"], s1)
    assert np.array_equal(scores[2]["w2c"], _w2cs([grid1[w1]]))
    match = [c for c in _log() if c["call"] == "match"][0]
    assert match["n"] == 2 and np.array_equal(match["query"].numpy(), ref.describe(depth.numpy()))
    assert np.array_equal(scores[3]["w2c"], _w2cs(grid2)) and np.array_equal(scores[3]["counts"], s2)
    assert np.array_equal(scores[4]["w2c"], _w2cs([KID])) and all(c["rows"] == n0 for c in scores)
    # three runs: the hold start, the grid's winner, the place grid's winner; the last one is kept
    loads = [load for t in _Tracker.made for load in t.loads][-3:]
    assert [torch.equal(a["tar_c2w"], b) for a, b in zip(loads, (FAR, grid1[w1], KID))] == [True] * 3
    assert (r.lost, r.relocalised, r.recognised, r.steps, r.best_step) == (False, True, 0, 36, 7)
    assert (r.tested, r.agree, r.front) == tuple(s2[0].tolist()) and torch.equal(r.c2w, KID) and r.eT == 0.0
    assert torch.equal(r.init_c2w, KID) and torch.equal(loc.trajectory[-1], KID)
    insert = [c for c in _log() if c["call"] == "insert"][0]
    assert torch.equal(insert["c2w"], KID) and r.added == H and r.map_size == n0 + H == loc.map.n_live
    # 7.1 degrees from keyframe 0: the frame is a keyframe itself, after its insertion
    assert r.keyframe == 2 and loc.map.n_keyframes == 3 and torch.equal(loc.map.keyframe_poses[2], KID)


def test_a_third_run_that_is_rejected_leaves_the_frame_lost_with_the_best_pose(monkeypatch):
    """More rows are asked for than the map has: nothing is ever accepted.  The frame at FAR is lost (and leaves the
    trajectory at FAR), the kidnapped frame is tracked three times, stays lost and leaves the map alone, and of the
    three estimates the one with the largest agree - front is handed on: the place grid's."""
    loc, grown = _grown(monkeypatch, keyframes=True, reloc_min_tested=4 * W * H + 1)
    assert grown.lost and grown.keyframe is None and grown.recognised == -1 and loc.map.n_keyframes == 1
    before = loc.map.points.clone()
    r = loc.track(*_frame_at(KID, 2), gt_c2w=KID)
    assert _calls("score", "match", "insert") == ["score", "score", "score", "match", "score", "score"]
    assert _sizes() == [1, PER_BASE, 1, PER_BASE, 1]  # one keyframe, one base
    margins = [int(c["counts"][0, 1] - c["counts"][0, 2]) for c in _log() if c["call"] == "score" and len(c["w2c"]) == 1]
    assert margins[2] > max(margins[:2])
    assert (r.lost, r.relocalised, r.recognised, r.keyframe, r.steps) == (True, False, -1, None, 36)
    assert torch.equal(r.c2w, KID) and torch.equal(loc.trajectory[-1], KID) and r.agree - r.front == margins[2]
    assert r.added == 0 and r.map_size == loc.map.n_live == before.shape[0] and torch.equal(loc.map.points, before)
    assert loc.map.n_keyframes == 1


def test_nothing_is_matched_when_the_second_run_is_accepted(monkeypatch):
    """The flow of tests/test_map_score_cpu.py -- a camera that has moved back by one step of the grid -- with keyframes
    on: the grid's winner is accepted, so no descriptor of the frame is made and nothing is matched."""
    first = torch.eye(4)
    loc = _localizer(monkeypatch, first, keyframes=True)
    score_cpu._ScoreMirrorMap.log = []
    truth = score_cpu._shift(2, -STEP)
    r = loc.track(*_frame_at(truth, 1), gt_c2w=truth)
    assert _calls("score", "match", "insert") == ["score", "score", "score", "insert"] and _sizes() == [1, PER_BASE, 1]
    assert (r.lost, r.relocalised, r.recognised, r.steps) == (False, True, -1, 24) and torch.equal(r.c2w, truth)
    assert r.keyframe == 1 and _calls()[-1] == "describe"  # 0.4 m from keyframe 0


def test_with_the_option_off_the_same_frame_is_lost(monkeypatch):
    loc, grown = _grown(monkeypatch)
    assert (grown.lost, grown.keyframe, grown.recognised) == (False, None, None)
    before = loc.map.points.clone()
    r = loc.track(*_frame_at(KID, 2), gt_c2w=KID)
    assert _calls() == ["score", "score", "score"] and _sizes() == [1, PER_BASE, 1]
    assert (r.lost, r.relocalised, r.recognised, r.keyframe, r.steps) == (True, False, None, None, 24)
    assert r.added == 0 and torch.equal(loc.map.points, before) and loc.map._place is None and loc.map.n_keyframes == 0
    out = LocalizeResult(torch.eye(4), torch.eye(4), 1, 1, 0.0, False)
    assert out.recognised is None and out.keyframe is None


# ---- the evaluation driver --------------------------------------------------------------------------------------------
def test_the_options_of_the_evaluation_driver_need_the_relocalisation(tmp_path, capsys):
    from gsplatloc_amd import eval as ev

    with pytest.raises(ValueError, match="map_keyframes"):
        ev.evaluate_room(None, 200, 3, sequential=True, map_mode=True, map_keyframes=True)
    with pytest.raises(ValueError, match="map_keyframes"):
        ev.evaluate_room(None, 200, 3, sequential=True, map_mode=True, map_reloc=True, map_keyframe_trans=0.1)
    with pytest.raises(ValueError, match="map_reloc"):
        ev.evaluate_room(None, 200, 3, sequential=True, map_keyframes=True)
    for extra, needs in ((["--map-keyframes"], "--map-reloc"), (["--sequential", "--map", "--map-keyframes"], "--map-reloc"),
                         (["--sequential", "--map", "--map-reloc", "--map-keyframe-rot-deg", "3"], "--map-keyframes"),
                         (["--sequential", "--map", "--map-reloc", "--map-keyframe-trans", "0.1"], "--map-keyframes"),
                         (["--map-keyframes", "--map-reloc"], "--map")):
        with pytest.raises(SystemExit):
            ev.main(["--root", str(tmp_path)] + extra)
        assert f"needs {needs}" in capsys.readouterr().err


# ---- the kernels' budget ----------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_the_place_kernels_stay_in_registers():
    """k_map_place_describe and k_map_place_match: no scratch, no accumulation registers, eight waves per SIMD; the
    descriptor's two LDS words, none for the match."""
    res = _resources("map_place.hip")
    describe = [v for k, v in res.items() if "k_map_place_describe" in k]
    match = [v for k, v in res.items() if "k_map_place_match" in k]
    assert len(describe) == 1 and len(match) == 1
    for r, lds in ((describe[0], 8), (match[0], 0)):
        assert r["ScratchSize"] == 0 and r["AGPRs"] == 0 and r["Occupancy"] == 8 and r["LDS"] == lds, r
