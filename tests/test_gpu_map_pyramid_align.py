"""GPU: coarse-to-fine alignment, GaussianMap.align_pose / align_poses / loop_constraint with levels= (csrc/map_pyramid.hip
under the entry points of csrc/map_align.hip and csrc/map_align_batch.hip), against the numpy mirror
tests/map_pyramid_ref.py on the fine-textured wall at 160 x 120.

The map is the frame at the identity, inserted by the map's own kernel; the mirror reads the rows back.  From the
identity, with the truth 0.1 m and 0.2 m (4 and 8 pixels) away: levels=3 gives the mirror's pose, working pose, and
every level's history integers and xi bit for bit, ends within 2e-4 m and 0.02 degrees with level 0 CONVERGED, and the
same start with levels=0 ends more than 0.02 m off.  levels=0 and levels=None are the call without the argument;
a batch equals its single calls; a loop constraint equals the alignment on the prefix; a prebuilt pyramid equals the one
built inside the call."""
import math

import numpy as np
import pytest
import torch

from gsplatloc_amd.mapping import ALIGN_STATUS, GaussianMap, MapConfig
from tests import map_photo_ref as photo
from tests import map_pyramid_ref as ref
from tests.map_align_batch_ref import done_of
from tests.test_map_pyramid_cpu import FAR, NEAR_R, NEAR_T

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
NEAR = 0.01
KEEP, BEYOND, KAPPA = photo.keep_of(0.05), photo.beyond_of(0.05), F32(1e-3)
SCALE, RMAX = 0.2, 0.1
PARAMS = (8, 1e-3, 7, math.radians(12.8), 0.32, math.radians(1.5e-4), 3e-5)  # MapConfig's defaults
W, H = photo.WALL_W, photo.WALL_H
K = torch.tensor([[photo.WALL_INTR[0], 0.0, photo.WALL_INTR[2]], [0.0, photo.WALL_INTR[1], photo.WALL_INTR[3]],
                  [0.0, 0.0, 1.0]])


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.fixture(scope="module")
def wall():
    """The map of the frame at the identity, its rows read back, and the two query frames with their mirrors."""
    m = GaussianMap(W, H, MapConfig(origins=True, align=True, photo_scale=SCALE, photo_max_residual=RMAX), DEV)
    d0, rgb0 = ref.fine_wall_frame(np.eye(4))
    assert m.insert_frame(torch.from_numpy(d0), torch.from_numpy(rgb0), K, torch.eye(4), origin=0) == (W * H, W * H)
    means, colors = m.points.cpu().numpy(), m.point_colors.cpu().numpy()
    cases = {}
    for t in (0.1, 0.2):
        c = ref.fine_wall_case(t)
        c["depth_t"], c["image_t"] = torch.from_numpy(c["depth"]).to(DEV), m.intensity(torch.from_numpy(c["rgb"]))
        assert np.array_equal(c["image_t"].cpu().numpy().view(np.uint32), c["image"].view(np.uint32))
        c["mirror"] = ref.pose_align(means, colors, np.eye(4, dtype=F32), c["intr"], c["depth"], c["image"], KEEP, BEYOND,
                                     KAPPA, NEAR, SCALE, RMAX, *PARAMS, levels=3)
        cases[t] = c
    return dict(map=m, means=means, colors=colors, cases=cases)


def _same_history(history, hist, xis, what):
    assert [(ALIGN_STATUS.index(s), u, t) for s, u, t, _, _ in history] == [tuple(r[:3]) for r in hist.tolist()], what
    assert [r for _, _, _, r, _ in history] == [float(r[3]) / 2.0 ** 20 for r in hist.tolist()], what
    assert all(np.array_equal(_u64(x), _u64(want)) for (_, _, _, _, x), want in zip(history, xis)), what


def _same_alignment(a, b, what):
    assert np.array_equal(_u64(a.w2c64), _u64(b.w2c64)) and torch.equal(a.c2w, b.c2w), what
    assert (a.status, a.steps, a.used, a.tested, a.level_steps) == (b.status, b.steps, b.used, b.tested, b.level_steps), what
    for ha, hb in zip([a.history] + (a.level_history or []), [b.history] + (b.level_history or [])):
        assert len(ha) == len(hb), what
        for ra, rb in zip(ha, hb):
            assert ra[:4] == rb[:4] and np.array_equal(_u64(ra[4]), _u64(rb[4])), what
    assert (a.level_history is None) == (b.level_history is None), what


@pytest.mark.parametrize("t", [0.1, 0.2])
def test_three_levels_against_the_mirror_and_the_basin(t, wall, capsys):
    """MI355X: the figures of the mirror (NOTES.md, "Image pyramid"), bit for bit."""
    m, c = wall["map"], wall["cases"][t]
    mirror = c["mirror"]
    got = m.align_pose(c["depth_t"], K, torch.eye(4), NEAR, intensity=c["image_t"], levels=3)
    assert len(got.level_history) == 4 and got.level_steps == [r[2] for r in mirror]
    for history, r in zip(got.level_history, mirror):
        _same_history(history, r[4], r[5], t)
    assert all(a[:4] == b[:4] for a, b in zip(got.history, got.level_history[-1]))  # the fields are level 0's
    assert np.array_equal(_u64(got.w2c64[:3]), _u64(mirror[-1][0]))
    assert got.status == "CONVERGED" and got.steps == mirror[-1][2]
    # the working pose of every level, from the launch itself: what the next level started at
    frames = m._level_frames(c["depth_t"], photo.WALL_INTR, (c["image_t"], SCALE, RMAX), 3, None, float(KEEP))
    start = torch.eye(4)
    per_level = m._align_levels_launch(frames, start, float(KEEP), float(BEYOND), float(KAPPA), NEAR, PARAMS[0],
                                       PARAMS[0], *PARAMS[1:])
    for (P, work, taken, hist, xis), r in zip(per_level, mirror):
        assert np.array_equal(_u64(P), _u64(r[0])) and np.array_equal(work.view(np.uint32), r[1].view(np.uint32))
        assert taken == r[2] and np.array_equal(hist, r[4]) and np.array_equal(_u64(xis), _u64(r[5]))
    err = photo.pose_error(got.w2c64, c["truth"])
    one = m.align_pose(c["depth_t"], K, torch.eye(4), NEAR, intensity=c["image_t"], levels=0)
    err_one = photo.pose_error(one.w2c64, c["truth"])
    with capsys.disabled():
        print(f"\n[pyramid] wall t = {t}: levels 3 -> 0 {err[0]:.3e} m {err[1]:.4f} deg, steps per level "
              f"{got.level_steps}; one level {err_one[0]:.3e} m {err_one[1]:.4f} deg ({one.status})")
    assert err[0] <= NEAR_T and err[1] <= NEAR_R
    assert err_one[0] > FAR and one.level_history is None and one.level_steps is None


def test_levels_zero_and_none_are_the_call_without_the_argument(wall):
    m, c = wall["map"], wall["cases"][0.1]
    before = (set(m._align_levels), set(m._align_batch_levels))
    for kw in (dict(), dict(intensity=c["image_t"])):
        plain = m.align_pose(c["depth_t"], K, torch.eye(4), NEAR, **kw)
        batch = m.align_poses(c["depth_t"], K, [torch.eye(4)], NEAR, **kw)[0]
        for levels in (0, None):
            _same_alignment(m.align_pose(c["depth_t"], K, torch.eye(4), NEAR, levels=levels, **kw), plain, (levels, kw))
            again = m.align_poses(c["depth_t"], K, [torch.eye(4)], NEAR, levels=levels, **kw)[0]
            _same_alignment(again, batch, (levels, kw))
            assert again.closed == batch.closed and plain.level_history is None
    assert (set(m._align_levels), set(m._align_batch_levels)) == before  # nothing of the pyramid was allocated


def test_a_batch_is_its_single_calls(wall):
    m, c = wall["map"], wall["cases"][0.1]
    starts = [torch.eye(4), torch.from_numpy(photo.twist_pose([0, 0, 1e-3, 0.02, 0.01, 0])).float(),
              torch.from_numpy(photo.twist_pose([1e-3, -1e-3, 0, -0.03, 0.0, 0.005])).float()]
    kw = dict(intensity=c["image_t"], levels=2, level_steps=4)
    batch = m.align_poses(c["depth_t"], K, starts, NEAR, **kw)
    w2cs = np.stack([np.linalg.inv(s.double().numpy()).astype(F32) for s in starts])
    wants = ref.pose_align_batch(wall["means"], wall["colors"], w2cs, c["intr"], c["depth"], c["image"], KEEP, BEYOND,
                                 KAPPA, NEAR, SCALE, RMAX, *PARAMS, levels=2, level_steps=4)
    for p, (got, start, want) in enumerate(zip(batch, starts, wants)):
        _same_alignment(got, m.align_pose(c["depth_t"], K, start, NEAR, **kw), p)
        alone = m.align_poses(c["depth_t"], K, [start], NEAR, **kw)[0]
        _same_alignment(got, alone, (p, "alone"))
        assert got.closed == alone.closed == (want[-1][3] == 2) == (done_of(want[-1][4]) == 2), p
        if got.closed:
            assert np.array_equal(got.final.H, alone.final.H) and np.array_equal(got.final.g, alone.final.g)
            assert got.final.used == alone.final.used == int(want[-1][6][28])
        assert [len(h) for h in got.level_history] == [4, 4, 8]
        for history, r in zip(got.level_history, want):
            _same_history(history, r[4], r[5], p)
        assert np.array_equal(_u64(got.w2c64[:3]), _u64(want[-1][0]))
    assert any(a.closed for a in batch)
    # the geometric batch takes levels as well, and equals its single call
    geo = m.align_poses(c["depth_t"], K, starts[:2], NEAR, levels=2)
    for got, start in zip(geo, starts):
        _same_alignment(got, m.align_pose(c["depth_t"], K, start, NEAR, levels=2), "geometric")


def test_a_loop_constraint_and_a_prebuilt_pyramid(wall):
    m, c = wall["map"], wall["cases"][0.2]
    kw = dict(intensity=c["image_t"], levels=2)
    n = m.rows_up_to(0)
    assert n == W * H
    want = m.align_pose(c["depth_t"], K, torch.eye(4), NEAR, rows=n, **kw)
    got = m.loop_constraint(c["depth_t"], K, torch.eye(4), 0, NEAR, **kw)
    _same_alignment(got.alignment, want, "loop")
    assert got.rows == n and len(got.alignment.level_history) == 3
    # a prebuilt pyramid, deeper than the call needs, photometric and geometric
    pyr = m.pyramid(c["depth_t"], 3, intensity=c["image_t"])
    _same_alignment(m.align_pose(c["depth_t"], K, torch.eye(4), NEAR, pyramid=pyr, **kw),
                    m.align_pose(c["depth_t"], K, torch.eye(4), NEAR, **kw), "prebuilt")
    _same_alignment(m.align_poses(c["depth_t"], K, [torch.eye(4)], NEAR, pyramid=pyr, **kw)[0],
                    m.align_poses(c["depth_t"], K, [torch.eye(4)], NEAR, **kw)[0], "prebuilt, batch")
    depth_only = m.pyramid(c["depth_t"], 2)
    _same_alignment(m.align_pose(c["depth_t"], K, torch.eye(4), NEAR, levels=2, pyramid=depth_only),
                    m.align_pose(c["depth_t"], K, torch.eye(4), NEAR, levels=2), "prebuilt, geometric")
    with pytest.raises(ValueError, match="holds no intensities"):
        m.align_pose(c["depth_t"], K, torch.eye(4), NEAR, pyramid=depth_only, **kw)
