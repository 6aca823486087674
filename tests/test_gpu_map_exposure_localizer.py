"""GPU: exposure compensation in Localizer(mode="map") (MapConfig.photo_exposure) on real kernels, at 160x120.

(a) The wall slide of tests/test_gpu_map_photo_localizer.py -- 6 frames, 1 cm per frame in the wall's plane,
    motion="hold", align, align_accept, info, photo_scale 0.2, the real tracker with 300 steps at the most -- with frame
    k's image g_k rgb + 255 b_k: frame 0 at (1, 0), the others at the EXPOSURES below, gains 0.8 .. 1.1 and offsets
    -0.03 .. 0.06 chosen so that every intensity stays inside (0.02, 0.98) (the texture lies in 0.1 .. 0.9).  Three runs:
    A constant exposure, B varying exposure without the option, C varying exposure with it.  C reports the inverse
    exposure (1 / g_k, -b_k / g_k) within 1e-2 with status OK on every frame; from the third frame on its translation
    error is at most half of B's at the same frame and at most three times A's; and the map's colours after C differ
    from those after A by less than those after B do.  Both factors are margins over yardstick runs.
(b) photo_exposure=False is the run without the field, bit for bit, on the box-room sequence.

Measured on the MI355X: the docstring of the test and NOTES.md, "Exposure compensation", where the numpy mirrors'
figures for this slide stand beside them."""
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
OPTIONS = dict(align=True, align_accept=True, info=True, photo_scale=0.2)
# (g_k, b_k) of frames 0 .. 5: the darkest intensity is 0.8 * 0.1 + 0.04 = 0.12, the brightest 1.1 * 0.9 - 0.03 = 0.96
EXPOSURES = [(1.0, 0.0), (0.85, 0.06), (1.1, -0.03), (0.8, 0.04), (1.05, 0.02), (0.9, -0.03)]


def _wall_run(exposures, **options):
    fx, fy, cx, cy = ref.WALL_INTR
    K = torch.tensor([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
    poses, frames = [], []
    for k in range(FRAMES):
        pose = np.eye(4)
        pose[0, 3] = STEP * k
        depth, rgb = ref.wall_frame(pose)
        g, b = exposures[k]
        rgb = (np.float32(g) * rgb + np.float32(255.0 * b)).astype(np.float32)
        y = ref.intensity(rgb)
        assert 0.02 < y.min() and y.max() < 0.98
        poses.append(torch.from_numpy(pose).float())
        frames.append((torch.from_numpy(depth), torch.from_numpy(rgb)))
    loc = Localizer(K, W, H, TrackerConfig(max_steps=TRACKER_STEPS), motion="hold", device=DEV, mode="map",
                    map_config=MapConfig(**OPTIONS, **options))
    loc.reset(*frames[0], poses[0])
    return loc, [loc.track(*frames[k], gt_c2w=poses[k]) for k in range(1, FRAMES)]


def _colour_distance(a, b):
    """Mean absolute difference of two maps' colours, row by row where the row counts agree; otherwise the difference
    of their mean intensities."""
    ca, cb = a.map.point_colors, b.map.point_colors
    if ca.shape == cb.shape:
        return float((ca - cb).abs().mean())
    return abs(float(ca.mean()) - float(cb.mean()))


def test_a_varying_exposure_is_estimated_and_compensated(capsys):
    """The three error series, the reported pairs and the two colour distances are printed; the mirrors' figures for the
    same slide are in NOTES.md, "Exposure compensation".  MI355X: A eT 7.11e-6, 1.03e-5, 5.79e-6, 1.25e-5, 9.39e-6 m; B
    2.11e-3, 5.80e-4, 2.59e-2, 4.67e-4, 3.87e-2 m (frames 3 and 5 fall back to the tracker); C 1.22e-5, 4.55e-6, 5.32e-6,
    1.00e-5, 5.30e-6 m, every frame direct, every estimate OK on 19 200 .. 19 440 rows and within 9.3e-4 of the inverse;
    map colours against A: B 9.73e-5, C 1.70e-6.  With the single estimate at the start pose frame 4 of C stood at
    3.86e-5 m, 3.1 x A -- the estimate had read the neighbouring pixels; hence ``Localizer._realigned``."""
    loc_a, run_a = _wall_run([(1.0, 0.0)] * FRAMES)
    loc_b, run_b = _wall_run(EXPOSURES)
    loc_c, run_c = _wall_run(EXPOSURES, photo_exposure=True)
    d_b, d_c = _colour_distance(loc_b, loc_a), _colour_distance(loc_c, loc_a)
    with capsys.disabled():
        for name, run in (("A constant", run_a), ("B varying", run_b), ("C compensated", run_c)):
            print(f"[exposure] wall, {name}: eT {['%.3e' % r.eT for r in run]}, eR {['%.3e' % r.eR for r in run]}, direct "
                  f"{[r.direct for r in run]}, tracker steps {[r.steps for r in run]}, photo rows "
                  f"{[r.info_photo_used for r in run]}, rows {[r.map_size for r in run]}")
        print(f"[exposure] wall, C reports {[(round(r.exposure_gain, 5), round(r.exposure_offset, 5), r.exposure_status, r.exposure_used) for r in run_c]}"
              f"; wanted {[(round(1 / g, 5), round(-b / g, 5)) for g, b in EXPOSURES[1:]]}; map colours against A: B "
              f"{d_b:.3e}, C {d_c:.3e}")
    for run in (run_a, run_b):
        assert all(r.exposure_gain is None and r.exposure_offset is None and r.exposure_status is None
                   and r.exposure_used is None for r in run)
    assert loc_a.map._exposure is None and loc_b.map._exposure is None and loc_c.map._exposure is not None
    for k, (a, b, c) in enumerate(zip(run_a, run_b, run_c), 1):
        g, off = EXPOSURES[k]
        assert not c.lost and c.exposure_status == "OK" and c.exposure_used > 256, (k, c.exposure_status)
        assert abs(c.exposure_gain - 1.0 / g) <= 1e-2 and abs(c.exposure_offset + off / g) <= 1e-2, (
            k, c.exposure_gain, c.exposure_offset)
        if k >= 3:
            assert c.eT <= 0.5 * b.eT and c.eT <= 3.0 * a.eT, (k, a.eT, b.eT, c.eT)
    assert d_c < d_b, (d_c, d_b)


def test_the_option_off_is_the_run_without_the_field_bit_for_bit(seq_b):  # noqa: F811
    plain = _run(seq_b, MapConfig(**OPTIONS))
    off = _run(seq_b, MapConfig(**OPTIONS, photo_exposure=False))
    assert torch.equal(off["traj"], plain["traj"])
    for a, b in zip(off["results"], plain["results"]):
        assert torch.equal(a.c2w, b.c2w) and torch.equal(a.init_c2w, b.init_c2w)
        assert (a.steps, a.best_step, a.best_loss, a.added, a.map_size, a.lost, a.aligned, a.align_status, a.align_steps,
                a.direct, a.direct_reason, a.info_used, a.info_min_eig, a.weak, a.sigma_t, a.sigma_r) == (
            b.steps, b.best_step, b.best_loss, b.added, b.map_size, b.lost, b.aligned, b.align_status, b.align_steps,
            b.direct, b.direct_reason, b.info_used, b.info_min_eig, b.weak, b.sigma_t, b.sigma_r)
        assert np.array_equal(a.cov, b.cov) and a.info_photo_used == b.info_photo_used
        assert a.exposure_gain is None and a.exposure_offset is None and a.exposure_status is None and a.exposure_used is None
    assert torch.equal(off["loc"].map.points, plain["loc"].map.points)
    assert torch.equal(off["loc"].map.point_colors, plain["loc"].map.point_colors)
    assert off["loc"].map._exposure is None  # no buffer, no launch
