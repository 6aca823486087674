"""A map with a resolution (MapConfig.merge_voxel), the parts that need no GPU: the validation of the two options, the
numpy mirror tests/map_merge_ref.py of the rule on hand-made cases, the argument checks of the two entry points and the
size of the workspace, GaussianMap.merge and Localizer(mode="map") around a map whose device calls are the mirrors."""
import ctypes

import numpy as np
import pytest
import torch

from gsplatloc_amd import _lib
from gsplatloc_amd.localizer import Localizer
from gsplatloc_amd.mapping import MapConfig
from gsplatloc_amd.my_gsplat import TrackerConfig
from gsplatloc_amd.synthetic import replica_intrinsics
from tests import map_merge_ref as ref
from tests import test_map_cpu as base
from tests.test_map_cpu import H, W, sequence  # noqa: F401  (the fixture)

F32 = np.float32
BAD_ARG, WORKSPACE = -1, -2  # GSL_ERR_BAD_ARG, GSL_ERR_WORKSPACE


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- MapConfig ------------------------------------------------------------------------------------------------------
def test_config_validation():
    assert MapConfig().merge_voxel is None and MapConfig().merge_every == 1
    cfg = MapConfig(merge_voxel=0.01, merge_every=3)
    assert cfg.merge_voxel == 0.01 and cfg.merge_every == 3
    MapConfig(merge_voxel=1)  # a whole number of metres is a length
    for bad in (0.0, -0.01, float("nan"), float("inf"), 1e-46, "0.01", True):
        with pytest.raises(ValueError, match="merge_voxel"):
            MapConfig(merge_voxel=bad)
    # 100 m / (2^20 - 1) = 9.54e-5 m: below it a 100 m scene leaves the cell range of the key
    with pytest.raises(ValueError, match="21 bits"):
        MapConfig(merge_voxel=9.0e-5)
    MapConfig(merge_voxel=1.0e-4)
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="merge_every"):
            MapConfig(merge_voxel=0.01, merge_every=bad)


# ---- the mirror of the rule -----------------------------------------------------------------------------------------
def test_two_rows_in_one_voxel():
    # h = 0.25 and every number below are exact in float32: f = (1.25, 2.5, -0.75), (1.75, 2.75, -0.25);
    # cells (1, 2, -1); fractions (0.25, 0.5, 0.25) and (0.75, 0.75, 0.75); mean fraction (0.5, 0.625, 0.5)
    means = np.array([[0.3125, 0.625, -0.1875], [0.4375, 0.6875, -0.0625]], F32)
    colors = np.array([[0.0, 1.0, 0.25], [1.0, 1.0, 0.75]], F32)
    stamps = np.array([9, 4], np.int32)
    r = ref.merge(means, colors, stamps, 0.25)
    assert r["counters"] == (1, 1, 1, 0) and r["ids"].tolist() == [0] and r["kept"].tolist() == [True, False]
    assert r["means"].tolist() == [[(1 + 0.5) * 0.25, (2 + 0.625) * 0.25, (-1 + 0.5) * 0.25]]
    assert r["colors"].tolist() == [[0.5, 1.0, 0.5]] and r["stamps"].tolist() == [9] and r["k_of"].tolist() == [2]
    # the other way round the first row is still row 0, and the result is the same
    r2 = ref.merge(means[::-1], colors[::-1], stamps[::-1], 0.25)
    assert np.array_equal(_u32(r2["means"]), _u32(r["means"])) and np.array_equal(_u32(r2["colors"]), _u32(r["colors"]))
    assert r2["stamps"].tolist() == [9] and r2["ids"].tolist() == [0]


def test_faces_negative_coordinates_and_minus_zero():
    h = 0.25
    means = np.array([[3 * h, 0.0, 0.0],  # on the face between cells 2 and 3 of x: cell 3, fraction 0
                      [3 * h + 0.125, 0.1, 0.1],  # the same voxel (3, 0, 0)
                      [np.nextafter(F32(3 * h), F32(0)), 0.0, 0.0],  # a float32 step below the face: cell 2
                      [-0.0, -0.0, -0.0],  # floor(-0) = -0: cell 0, with rows 4 and 5
                      [0.0, 0.0, 0.0],
                      [0.1, 0.1, 0.1],
                      [-0.1, -0.1, -0.1],  # floor, not truncation: cell -1, alone
                      [-h, -h, -h],  # on a face at a negative coordinate: cell -1 as well, fraction 0
                      ], F32)
    mergeable, c, q, key = ref.cells(means, ref.h_of(h)[0])
    assert mergeable.all()
    assert c.tolist() == [[3, 0, 0], [3, 0, 0], [2, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [-1, -1, -1], [-1, -1, -1]]
    assert q[0].tolist() == [0, 0, 0] and q[3].tolist() == [0, 0, 0] and q[7].tolist() == [0, 0, 0]
    assert q[2, 0] == 65536  # the fraction of the row below the face rounds to a whole cell, the cell stays 2
    r = ref.merge(means, np.zeros((8, 3), F32), np.arange(8, dtype=np.int32), h)
    assert r["ids"].tolist() == [0, 2, 3, 6] and r["k_of"].tolist() == [2, 1, 3, 2]
    assert r["stamps"].tolist() == [1, 2, 5, 7]
    assert np.array_equal(_u32(r["means"][1]), _u32(means[2]))  # a singleton keeps its bits
    # voxel (-1, -1, -1): fractions 0.6 (of -0.1 / 0.25 = -0.4) and 0: the mean lies inside the voxel
    assert (-h <= r["means"][3]).all() and (r["means"][3] < 0).all()


def test_rows_that_are_not_mergeable_keep_their_place_and_bits():
    h = 0.5
    far = float(F32(2 ** 20) * F32(h))  # cell 2^20: one beyond the key's range
    edge = float(F32(2 ** 20 - 1) * F32(h))  # the last cell inside it
    means = np.array([[1.1, 1.1, 1.1], [np.nan, 1.1, 1.1], [1.2, 1.2, 1.2], [np.inf, 0.0, 0.0], [1.1, -np.inf, 1.1],
                      [far, 0.0, 0.0], [far, 0.0, 0.0], [-far - 1.0, 0.0, 0.0], [edge, 0.1, 0.1], [edge, 0.2, 0.2],
                      [np.nan, np.nan, np.nan], [np.nan, np.nan, np.nan], [-edge, 0.0, 0.0]], F32)
    colors = np.full((13, 3), 0.5, F32)
    colors[1, 0] = np.nan
    stamps = np.arange(13, dtype=np.int32)
    mergeable = ref.cells(means, ref.h_of(h)[0])[0]
    assert mergeable.tolist() == [True, False, True, False, False, False, False, False, True, True, False, False, True]
    r = ref.merge(means, colors, stamps, h)
    assert r["ids"].tolist() == [0, 1, 3, 4, 5, 6, 7, 8, 10, 11, 12]  # only rows 2 and 9 went, into rows 0 and 8
    for at, old in enumerate(r["ids"]):
        if old not in (0, 8):
            assert np.array_equal(_u32(r["means"][at]), _u32(means[old])), old
            assert np.array_equal(_u32(r["colors"][at]), _u32(colors[old])) and r["stamps"][at] == stamps[old]
    assert r["stamps"][0] == 2 and r["stamps"][7] == 9
    assert r["counters"] == (11, 2, 11, 0)


def test_colours_eight_bit_exact_clamped_and_nan():
    means = np.zeros((3, 3), F32) + F32(0.1)
    colors = np.array([[7 / 255, -3.0, np.nan], [200 / 255, 0.5, 1.0], [255 / 255, 9.0, 0.5]], F32)
    units = ref.colour_units(colors)
    assert units[:, 0].tolist() == [7 * 256, 200 * 256, 255 * 256]  # 65280 = 255 * 256
    assert units[:, 1].tolist() == [0, 32640, 65280] and units[:, 2].tolist() == [0, 65280, 32640]
    r = ref.merge(means, colors, np.zeros(3, np.int32), 1.0)
    want = [F32((7 + 200 + 255) * 256 / (65280.0 * 3)), F32((0 + 32640 + 65280) / (65280.0 * 3)), F32(0.5)]
    assert r["colors"][0].tolist() == [float(w) for w in want]


@pytest.mark.parametrize("n", [1, 50, 1000])
def test_properties_on_a_random_cloud(n):
    rng = np.random.default_rng(n)
    means = rng.uniform(-1.0, 1.0, (n, 3)).astype(F32)
    colors = rng.uniform(-0.2, 1.2, (n, 3)).astype(F32)
    stamps = rng.integers(0, 50, n).astype(np.int32)
    h = 0.3
    r = ref.merge(means, colors, stamps, h)
    stay, removed, stored, flag = r["counters"]
    assert stay + removed == n and stored == stay == len(r["ids"]) and flag == 0
    assert (np.diff(r["ids"]) > 0).all()  # ascending old index: the map's order
    single = r["k_of"] == 1
    assert np.array_equal(_u32(r["means"][single]), _u32(means[r["ids"][single]]))  # singletons bit-identical
    assert np.array_equal(_u32(r["colors"][single]), _u32(colors[r["ids"][single]]))
    assert np.array_equal(r["stamps"][single], stamps[r["ids"][single]])
    assert int(r["k_of"].sum()) == n
    if n >= 50:
        assert (~single).any()
    # a fused row lies in its voxel (up to the rounding of the last step) and its colour in [0, 1]
    lo = np.floor(means[r["ids"]] * ref.h_of(h)[0]) * F32(h)
    assert (r["means"] >= lo - 1e-6).all() and (r["means"] <= lo + F32(h) + 1e-6).all()
    assert (r["colors"][~single] >= 0).all() and (r["colors"][~single] <= 1).all()
    # a permutation of the rows inside every voxel that keeps each voxel's first row fixed changes nothing
    mergeable, _, _, key = ref.cells(means, ref.h_of(h)[0])
    perm = np.arange(n)
    for k in np.unique(key[mergeable]):
        members = np.flatnonzero(mergeable & (key == k))
        if len(members) > 2:
            perm[members[1:]] = members[1:][rng.permutation(len(members) - 1)]
    r2 = ref.merge(means[perm], colors[perm], stamps[perm], h)
    for name in ("ids", "means", "colors", "stamps", "k_of"):
        assert np.array_equal(_u32(r2[name].astype(r[name].dtype)), _u32(r[name])), name
    assert ref.occupancy(means, h) == int(r["k_of"].max())
    assert ref.occupancy(means, 1e-4) == 1  # a voxel too small to share


# ---- the entry points, before any launch ----------------------------------------------------------------------------
def test_workspace_size():
    lib = _lib.load_library()

    def want(n):
        nb, slots = (n + 255) // 256, 2
        while slots < 2 * n:
            slots *= 2
        return 48 * nb + 16 + 16 * slots + 56 * n

    for n in (1, 2, 3, 256, 257, 4099, 307200):
        assert lib.gsl_map_merge_ws_bytes(n) == want(n), n
        assert lib.gsl_map_merge_ws_bytes(n) >= lib.gsl_map_view_ws_bytes(n)
    assert lib.gsl_map_merge_ws_bytes(0) == lib.gsl_map_merge_ws_bytes(-4) == lib.gsl_map_merge_ws_bytes(2 ** 31)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """The pointers are one dummy HOST buffer: a launch would give GSL_ERR_HIP or worse."""
    lib = _lib.load_library()
    buf = ctypes.create_string_buffer(256)
    p, n = ctypes.addressof(buf), 100
    full = lib.gsl_map_merge_ws_bytes(n)
    good = dict(means=p, colors=p, stamps=p, n_rows=n, inv_h=4.0, h=0.25, counters=p, ws=p, ws_bytes=full, stream=None)
    rows = [dict(means=None), dict(colors=None), dict(stamps=None), dict(counters=None), dict(ws=None), dict(n_rows=0),
            dict(n_rows=-1), dict(n_rows=2 ** 31), dict(h=0.0), dict(h=-0.25), dict(h=float("nan")),
            dict(h=float("inf")), dict(inv_h=0.0), dict(inv_h=float("inf")), dict(inv_h=float("nan")), dict(inv_h=-4.0)]
    for over in rows:
        assert lib.gsl_map_merge_select(*dict(good, **over).values()) == BAD_ARG, over
    assert lib.gsl_map_merge_select(*dict(good, ws_bytes=full - 1).values()) == WORKSPACE
    good = dict(ids=p, counters=p, n_rows=n, out_means=p, out_colors=p, out_stamps=p, ws=p, ws_bytes=full, stream=None)
    rows = [dict(ids=None), dict(counters=None), dict(out_means=None), dict(out_colors=None), dict(out_stamps=None),
            dict(ws=None), dict(n_rows=0), dict(n_rows=2 ** 31)]
    for over in rows:
        assert lib.gsl_map_merge_apply(*dict(good, **over).values()) == BAD_ARG, over
    assert lib.gsl_map_merge_apply(*dict(good, ws_bytes=full - 1).values()) == WORKSPACE
    assert not any(buf.raw)  # nothing wrote to the buffer


# ---- GaussianMap.merge and Localizer(mode="map") around the mirrors -------------------------------------------------
class _MergeMirrorMap(base._MirrorMap):
    """GaussianMap whose device calls are the numpy mirrors (host tensors)."""
    merges = 0

    def _merge_launch(self):
        _MergeMirrorMap.merges += 1
        n, f = self.n_live, self._free_buffers()
        r = ref.merge(self.means[:n].numpy(), self.colors[:n].numpy(), self.stamps[:n].numpy(), self.cfg.merge_voxel)
        k = len(r["ids"])
        f["means"][:k], f["colors"][:k] = torch.from_numpy(r["means"]), torch.from_numpy(r["colors"])
        f["stamps"][:k], f["ids"][:k] = torch.from_numpy(r["stamps"]), torch.from_numpy(r["ids"])
        return r["counters"]


def _filled(config, means, stamps=None):
    n = len(means)
    m = _MergeMirrorMap(W, H, config, "cpu")
    m.means[:n], m.colors[:n], m.n_live = torch.from_numpy(means), torch.from_numpy(means) * 0 + 0.5, n
    if stamps is not None:
        m.stamps[:n] = torch.from_numpy(stamps)
    return m


def test_merge_swaps_the_buffers_only_when_something_went():
    means = np.array([[0.1, 0.1, 0.1], [1.1, 0.1, 0.1], [0.2, 0.2, 0.2], [2.1, 0.1, 0.1]], F32)
    with pytest.raises(RuntimeError, match="merge_voxel"):
        _filled(MapConfig(), means).merge()
    m = _filled(MapConfig(merge_voxel=1.0, capacity=10), means, np.array([3, 5, 8, 1], np.int32))
    assert _MergeMirrorMap(W, H, MapConfig(merge_voxel=1.0), "cpu").merge() == (0, 0)  # an empty map
    mptr, m._view_rows = m.means.data_ptr(), 4
    assert m.merge() == (1, 3) and m.n_live == 3 and m.survivors.tolist() == [0, 1, 3]
    assert m.means.data_ptr() != mptr and m._free["means"].data_ptr() == mptr and m._view_rows == -1
    assert m.stamps[:3].tolist() == [8, 5, 1]
    assert torch.allclose(m.points[0], torch.tensor([0.15, 0.15, 0.15]), atol=1e-5)
    # nothing shares a voxel now: not a bit changes, the very same tensors stay
    mptr, before = m.means.data_ptr(), (m.means.clone(), m.colors.clone(), m.stamps.clone())
    m._view_rows = 3
    assert m.merge() == (0, 3) and m.means.data_ptr() == mptr and m._view_rows == 3
    assert torch.equal(m.means, before[0]) and torch.equal(m.colors, before[1]) and torch.equal(m.stamps, before[2])
    assert m.survivors.tolist() == [0, 1, 2]


def _localizer(tracker, config):
    tracker.made = base._Tracker.made = []
    _MergeMirrorMap.merges = 0
    return Localizer(replica_intrinsics(W, H), W, H, TrackerConfig(max_steps=5), normalize=False, motion="hold",
                     device="cpu", tracker_factory=tracker, mode="map", map_factory=_MergeMirrorMap,
                     map_renderer=base._Renderer(), map_config=config)


def test_the_localizer_merges_after_the_insertion(sequence, monkeypatch):  # noqa: F811
    import gsplatloc_amd.data.dataset as DS

    monkeypatch.setattr(DS, "compute_depth_gt", lambda pts, col, Ks, c2w, height, width: torch.zeros(height, width))
    frames = sequence
    # without the option: merged is None, as removed / evicted are, and merge is never called
    loc = _localizer(base._Tracker, MapConfig())
    loc.reset(*frames[0])
    r = loc.track(frames[1][0], frames[1][1], gt_c2w=frames[1][2])
    assert r.merged is None and r.removed is None and r.evicted is None and _MergeMirrorMap.merges == 0
    assert loc.merged_at_reset is None and r.map_size == W * H + H
    # with it: after reset's insertion and after every frame's; map_size is the count after the merge
    h = 0.2
    loc = _localizer(base._Tracker, MapConfig(merge_voxel=h))
    loc.reset(*frames[0])
    assert _MergeMirrorMap.merges == 1 and loc.merged_at_reset > 0 and loc.map.n_live == W * H - loc.merged_at_reset
    assert ref.occupancy(loc.map.points.numpy(), h) == 1  # fused rows do not leave their voxel
    sizes = [loc.map.n_live]
    for k in (1, 2, 3):
        r = loc.track(frames[k][0], frames[k][1], gt_c2w=frames[k][2])
        assert r.added == H and r.merged >= 0 and r.map_size == sizes[-1] + H - r.merged == loc.map.n_live
        assert _MergeMirrorMap.merges == 1 + k
        sizes.append(r.map_size)
    # the tracker sees the merged map (and is kept while its row count does not change)
    assert [ld["tar_points"].shape[0] for t in base._Tracker.made for ld in t.loads] == sizes[:-1]
    # every second frame
    loc = _localizer(base._Tracker, MapConfig(merge_voxel=h, merge_every=2))
    loc.reset(*frames[0])
    merged = [loc.track(frames[k][0], frames[k][1], gt_c2w=frames[k][2]).merged for k in (1, 2, 3, 4)]
    assert _MergeMirrorMap.merges == 3 and merged[0] == 0 and merged[2] == 0
    # a lost frame merges nothing
    loc = _localizer(base._LostTracker, MapConfig(merge_voxel=h))
    loc.reset(*frames[0])
    r = loc.track(frames[1][0], frames[1][1])
    assert r.lost and r.merged == 0 and _MergeMirrorMap.merges == 1
