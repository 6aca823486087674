"""GPU: the photometric term in Localizer(mode="map") (MapConfig.photo_scale) on real kernels, at 160x120.

(a) A camera sliding along the textured wall of tests/map_photo_ref.py, 1 cm per frame in the wall's plane, 6 frames,
    motion="hold", align=True, align_accept=True, info=True, the real tracker with 300 steps at the most.  The yardstick
    is the run with photo_scale=None: depth alone sees no motion along a wall, every frame is weak, the alignment stays
    where it started and the tracker (expected depth only) has nothing to pull it along the wall either.  With
    photo_scale=0.2 the translation error from the third frame on is at most half the yardstick's at the same frame (the
    float64 prototype says two orders of magnitude), no frame is weak and every frame reports photometric rows.
    Direct frames, step counts and errors of both runs are printed (NOTES.md, "Photometric term").
(b) The box-room constant twist of tests/test_gpu_map_localizer.py with the same options: photo_scale=0 is, bit for bit,
    the run without the field -- every Jc is zero, and the integers of the sums are the geometric ones.

Measured on the MI355X: the docstrings of the tests."""
import numpy as np
import pytest
import torch

from gsplatloc_amd.localizer import Localizer
from gsplatloc_amd.mapping import MapConfig
from gsplatloc_amd.my_gsplat import TrackerConfig
from tests import map_photo_ref as ref
from tests.test_gpu_map_align_localizer import _run
from tests.test_gpu_map_localizer import seq_b  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda"
W, H = ref.WALL_W, ref.WALL_H
FRAMES, STEP, TRACKER_STEPS = 6, 0.01, 300
OPTIONS = dict(align=True, align_accept=True, info=True)


def _wall_run(**photo):
    fx, fy, cx, cy = ref.WALL_INTR
    K = torch.tensor([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
    poses, frames = [], []
    for k in range(FRAMES):
        pose = np.eye(4)
        pose[0, 3] = STEP * k
        depth, rgb = ref.wall_frame(pose)
        poses.append(torch.from_numpy(pose).float())
        frames.append((torch.from_numpy(depth), torch.from_numpy(rgb)))
    loc = Localizer(K, W, H, TrackerConfig(max_steps=TRACKER_STEPS), motion="hold", device=DEV, mode="map",
                    map_config=MapConfig(**OPTIONS, **photo))
    loc.reset(*frames[0], poses[0])
    return loc, [loc.track(*frames[k], gt_c2w=poses[k]) for k in range(1, FRAMES)]


def test_colour_follows_a_camera_that_slides_along_a_wall(capsys):
    """MI355X: depth alone -- no direct frame (every one "weak"), 300 tracker steps each, eT 2.57e-2, 3.51e-2, 4.44e-2,
    5.41e-2, 6.37e-2 m; photo_scale 0.2 -- 5 of 5 frames direct after 4 alignment steps each, eT 7.1e-6 .. 1.25e-5 m,
    smallest eigenvalue of H / used 7.7e-3, 18 644 .. 18 880 photometric rows."""
    _, yard = _wall_run()
    loc, got = _wall_run(photo_scale=0.2)
    with capsys.disabled():
        for name, run in (("depth alone", yard), ("photo_scale 0.2", got)):
            print(f"[photo] wall, {name}: direct {[r.direct for r in run]} ({[r.direct_reason for r in run]}), align "
                  f"{[(r.align_status, r.align_steps) for r in run]}, tracker steps {[r.steps for r in run]}, eT "
                  f"{['%.3e' % r.eT for r in run]}, eR {['%.3e' % r.eR for r in run]}, weak {[r.weak for r in run]}, "
                  f"min eig {[r.info_min_eig for r in run]}, photo rows {[r.info_photo_used for r in run]}")
    assert all(r.info_photo_used is None for r in yard) and all(r.weak is not False for r in yard)
    assert all(r.direct is False for r in yard)  # the parent's behaviour: a wall is never accepted
    for k, (r, y) in enumerate(zip(got, yard), 1):
        assert not r.lost and r.weak is False and r.info_photo_used > 0 and r.info_photo_used <= r.info_used, k
        if k >= 3:
            assert r.eT <= 0.5 * y.eT, (k, r.eT, y.eT)
    assert loc.map._info_photo is not None and loc.map._info is None  # every call of the frame took the image


def test_scale_zero_is_the_run_without_the_field_bit_for_bit(seq_b):  # noqa: F811
    plain = _run(seq_b, MapConfig(**OPTIONS))
    zero = _run(seq_b, MapConfig(**OPTIONS, photo_scale=0.0))
    assert torch.equal(zero["traj"], plain["traj"])
    for a, b in zip(zero["results"], plain["results"]):
        assert torch.equal(a.c2w, b.c2w) and torch.equal(a.init_c2w, b.init_c2w)
        assert (a.steps, a.best_step, a.best_loss, a.added, a.map_size, a.lost, a.aligned, a.align_status, a.align_steps,
                a.direct, a.direct_reason, a.info_used, a.info_min_eig, a.weak, a.sigma_t, a.sigma_r) == (
            b.steps, b.best_step, b.best_loss, b.added, b.map_size, b.lost, b.aligned, b.align_status, b.align_steps,
            b.direct, b.direct_reason, b.info_used, b.info_min_eig, b.weak, b.sigma_t, b.sigma_r)
        assert np.array_equal(a.cov, b.cov) and b.info_photo_used is None and 0 < a.info_photo_used <= a.info_used
    assert torch.equal(zero["loc"].map.points, plain["loc"].map.points)
    assert torch.equal(zero["loc"].map.point_colors, plain["loc"].map.point_colors)
    assert any(r.direct for r in plain["results"])  # the options are at work in this run
