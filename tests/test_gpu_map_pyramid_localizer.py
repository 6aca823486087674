"""GPU: coarse-to-fine alignment in Localizer(mode="map") (MapConfig.align_levels) on real kernels, at 160 x 120, on the
fine-textured wall of tests/map_pyramid_ref.py (finest wavelength about 8.5 pixels).

(a) A camera sliding along the wall, 0.1 m (4 pixels) per frame in the wall's plane, 4 frames after the first,
    motion="hold", align=True, align_accept=True, photo_scale=0.2, the real tracker with 300 steps at the most.  With
    align_levels=3 every frame is direct: the alignment converged from 4 pixels off, and the map's rows pin the pose
    down.  The same run with align_levels=0 ends more than 0.02 m off, or lost: one level does not converge from there,
    and the tracker (expected depth only) has nothing to pull it along a wall.  Each frame's aligned start is, bit for
    bit, what GaussianMap.align_pose(levels=3) gives on the same map and frame.
(b) With align_levels=0 the other two fields are only numbers: the run is the one without them, bit for bit.

The per-frame error of the pyramid run has no mirror -- the loop feeds its own estimates back, and every frame's rows
go into the map at the estimated pose -- so the bound is four times the worst error measured on the MI355X (the
docstring of the test; NOTES.md, "Image pyramid")."""
import numpy as np
import pytest
import torch

from gsplatloc_amd.localizer import Localizer
from gsplatloc_amd.mapping import MapConfig
from gsplatloc_amd.my_gsplat import TrackerConfig
from tests import map_photo_ref as photo
from tests import map_pyramid_ref as ref
from tests.test_map_pyramid_cpu import FAR

pytestmark = pytest.mark.gpu
DEV = "cuda"
W, H = photo.WALL_W, photo.WALL_H
TRACKER_STEPS = 300
OPTIONS = dict(align=True, align_accept=True, photo_scale=0.2)
MEASURED_WORST_ET = 3.052e-7  # metres, the MI355X run of the docstring below
K = torch.tensor([[photo.WALL_INTR[0], 0.0, photo.WALL_INTR[2]], [0.0, photo.WALL_INTR[1], photo.WALL_INTR[3]],
                  [0.0, 0.0, 1.0]])


def _slide(frames, step, check=None, **options):
    """The run over frames 1 .. frames of a camera that moves step metres per frame along x.  check(loc, depth, rgb):
    called before every track, its results are returned as well."""
    poses, images = [], []
    for k in range(frames + 1):
        pose = np.eye(4)
        pose[0, 3] = step * k
        depth, rgb = ref.fine_wall_frame(pose)
        poses.append(torch.from_numpy(pose).float())
        images.append((torch.from_numpy(depth), torch.from_numpy(rgb)))
    loc = Localizer(K, W, H, TrackerConfig(max_steps=TRACKER_STEPS), motion="hold", device=DEV, mode="map",
                    map_config=MapConfig(**OPTIONS, **options))
    loc.reset(*images[0], poses[0])
    results, checks = [], []
    for k in range(1, frames + 1):
        if check is not None:
            checks.append(check(loc, *images[k]))
        results.append(loc.track(*images[k], gt_c2w=poses[k]))
    return loc, results, checks


def _direct_alignment(loc, depth, rgb):
    m = loc.map
    image = m.intensity(rgb.to(DEV))
    return m.align_pose(depth.to(DEV), K, loc.trajectory[-1], loc.cfg.gs.near_plane, intensity=image, levels=3)


def test_three_levels_follow_a_camera_that_slides_four_pixels_a_frame(capsys):
    """MI355X: align_levels=3 -- 4 of 4 frames direct, every alignment CONVERGED with 8, 8, 3, 2 steps from the coarsest
    level to the frame, no tracker step, eT 3.05e-7, 2.76e-7, 2.57e-7, 2.75e-7 m (the worst is MEASURED_WORST_ET), eR
    8.0e-6 .. 1.05e-5 degrees; align_levels=0 -- eT 0.113, 0.233, 0.315, 0.414 m, three frames STEPPED after 8 steps and
    handed to the tracker (300 steps each), and one CONVERGED on a neighbouring wave of the texture, 0.23 m off, and was
    taken as a direct frame: a basin that is too small does not only fail, it can fail silently."""
    loc, got, direct = _slide(4, 0.1, check=_direct_alignment, align_levels=3)
    _, yard, _ = _slide(4, 0.1)
    with capsys.disabled():
        for name, run in (("align_levels 3", got), ("align_levels 0", yard)):
            print(f"\n[pyramid] wall slide, {name}: direct {[r.direct for r in run]} ({[r.direct_reason for r in run]}), "
                  f"align {[(r.align_status, r.align_steps, r.align_level_steps) for r in run]}, tracker steps "
                  f"{[r.steps for r in run]}, lost {[r.lost for r in run]}, eT {['%.3e' % r.eT for r in run]}, eR "
                  f"{['%.3e' % r.eR for r in run]}")
    for k, (r, al) in enumerate(zip(got, direct), 1):
        assert r.direct is True and not r.lost and r.aligned is True, (k, r.direct_reason)
        # the frame's aligned start is the direct call's, bit for bit
        assert torch.equal(r.init_c2w, al.c2w.to(r.init_c2w.device)) and torch.equal(r.c2w, r.init_c2w), k
        assert (r.align_status, r.align_steps, r.align_level_steps) == (al.status, al.steps, al.level_steps), k
        assert len(r.align_level_steps) == 4 and r.align_status == "CONVERGED"
        assert r.eT <= 4.0 * MEASURED_WORST_ET, (k, r.eT)
    assert all(r.align_level_steps is None for r in yard)
    assert yard[-1].lost or yard[-1].eT > FAR, yard[-1].eT
    assert 4 in loc.map._align_batch_levels  # align_accept goes through the batched alignment, four levels of it


def test_levels_zero_is_the_run_without_the_fields_bit_for_bit():
    plain_loc, plain, _ = _slide(3, 0.01)
    zero_loc, zero, _ = _slide(3, 0.01, align_levels=0, align_level_steps=3, pyramid_rho=0.2)
    assert torch.equal(zero_loc.trajectory, plain_loc.trajectory)
    for a, b in zip(zero, plain):
        assert torch.equal(a.c2w, b.c2w) and torch.equal(a.init_c2w, b.init_c2w)
        assert (a.steps, a.best_step, a.best_loss, a.added, a.map_size, a.lost, a.aligned, a.align_status, a.align_steps,
                a.direct, a.direct_reason, a.align_level_steps) == (
            b.steps, b.best_step, b.best_loss, b.added, b.map_size, b.lost, b.aligned, b.align_status, b.align_steps,
            b.direct, b.direct_reason, None)
    assert torch.equal(zero_loc.map.points, plain_loc.map.points)
    assert torch.equal(zero_loc.map.point_colors, plain_loc.map.point_colors)
    assert not zero_loc.map._align_levels and not zero_loc.map._align_batch_levels  # nothing of the pyramid exists
    assert any(r.direct for r in plain)  # the options are at work in this run
