"""Sequential localisation, the parts that need no GPU: the constant-velocity hand-over against its existing torch mirror
and across the quaternion's two hemispheres, the way back from a pair's normalised frame, a pair placed with a given
pose, the Localizer's composition of all of them around a stand-in tracker, and the new entry point's argument check."""
import math

import pytest
import torch

from gsplatloc_amd.data import Parser
from gsplatloc_amd.data.normalize import align_principle_axes, denormalize_camera, transform_cameras
from gsplatloc_amd.localizer import Localizer, LocalizeResult, predict_pose
from gsplatloc_amd.my_gsplat import CameraOptModule_quat_tans, TrackerConfig, rotation_matrix_to_quaternion
from gsplatloc_amd.my_gsplat.geometry import depth_to_points
from gsplatloc_amd.my_gsplat.trainer import TrackResult, calculate_rotation_error
from gsplatloc_amd.synthetic import replica_intrinsics, write_replica_sequence
from tests.pose_ref import axis_angle

W, H, N_FRAMES = 32, 24, 7


def _pose(axis, deg, t=(0.0, 0.0, 0.0)):
    c2w = torch.eye(4, dtype=torch.float64)
    c2w[:3, :3] = axis_angle(axis, deg)
    c2w[:3, 3] = torch.tensor(t, dtype=torch.float64)
    return c2w.float()


def test_prediction_equals_the_mirrored_hand_over():
    """predict_pose on two world poses 0.4 degrees / 1 cm apart == CameraOptModule_quat_tans.update_pose(None) seeded
    with the first and moved to the second: both float32, the same formula -- 1e-6."""
    prev = _pose((0.3, -0.8, 0.5), 20.0, (0.5, -0.2, 0.3))
    step = _pose((0.2, 0.9, -0.4), 0.4, (0.006, -0.008, 0.0))
    cur = prev @ step
    assert abs(float(torch.norm(step[:3, 3])) - 0.01) < 1e-6
    cam = CameraOptModule_quat_tans(prev)
    cam.update_pose(cur)
    cam.update_pose(None)
    want = cam().detach()
    got = predict_pose(prev, cur)
    assert got.dtype == torch.float32 and got.shape == (4, 4)
    assert float((got - want).abs().max()) <= 1e-6, (got, want)
    # and it is where a constant twist leads: closer to the next pose than one tenth of a step
    nxt = cur @ step
    assert float(torch.norm(got[:3, 3] - nxt[:3, 3])) < 1e-3
    assert calculate_rotation_error(got, nxt) < 0.04


def test_prediction_across_the_quaternion_hemispheres():
    """Two poses 0.4 degrees apart, both a 179.9 degree rotation, about axes (cos a, -sin a, 0) on either side of
    a = 45 degrees: the conversion takes its m00 branch (x > 0) for one and its m11 branch (y > 0) for the other, so the
    two quaternions come out with opposite signs (the precondition, asserted).  The prediction stays within twice the
    inter-frame rotation of the current pose, and it lands on the continued motion cur (prev^-1 cur): the extrapolation
    is linear in the quaternion, so its error is of second order in the step (7e-3 rad squared, far below a quarter of
    the step).  Differenced as they come the two quaternions give 3 q_cur - (q_cur + q_prev'), a third of a step BACK
    from the current pose and 4/3 of a step from the continued motion, which the second bound refuses (shown below)."""
    def about(a_deg):
        a = math.radians(a_deg)
        return (math.cos(a), -math.sin(a), 0.0)

    prev, cur = _pose(about(44.9), 179.9), _pose(about(45.1), 179.9, (0.01, 0.0, 0.0))
    q_prev = rotation_matrix_to_quaternion(prev[:3, :3].contiguous())
    q_cur = rotation_matrix_to_quaternion(cur[:3, :3].contiguous())
    assert float((q_prev * q_cur).sum()) < -0.99, (q_prev, q_cur)  # opposite hemispheres
    step = calculate_rotation_error(prev, cur)
    assert abs(step - 0.4) < 1e-2
    got = predict_pose(prev, cur)
    off = calculate_rotation_error(got, cur)
    assert off <= 2.0 * step, (off, step)
    ahead = cur @ (torch.linalg.inv(prev.double()) @ cur.double()).float()
    miss = calculate_rotation_error(got, ahead)
    assert miss <= 0.25 * step, (miss, step)
    assert float(torch.norm(got[:3, 3] - torch.tensor([0.02, 0.0, 0.0]))) <= 1e-7
    # without the sign alignment (the mirror differences its parameters as they are)
    cam = CameraOptModule_quat_tans(prev)
    cam.update_pose(cur)
    cam.update_pose(None)
    naive = calculate_rotation_error(cam().detach(), ahead)
    print(f"hemisphere: step {step:.4f} deg; off the continued motion: aligned {miss:.5f} deg, unaligned {naive:.4f} deg")
    assert naive > step


def test_denormalize_camera_round_trip():
    g = torch.Generator().manual_seed(3)
    cloud = torch.randn(500, 3, generator=g) * torch.tensor([2.0, 0.7, 1.3]) + torch.tensor([0.4, -1.1, 2.0])
    T = align_principle_axes(cloud)
    c2w = _pose((0.5, 0.4, -0.7), 140.0, (1.2, -0.7, 0.4))
    back = denormalize_camera(T, transform_cameras(T, c2w.unsqueeze(0))[0].squeeze(0))
    assert back.dtype == torch.float32
    assert float((back - c2w).abs().max()) <= 1e-6, (back, c2w)


@pytest.fixture(scope="module")
def sequence(tmp_path_factory):
    root = tmp_path_factory.mktemp("seq")
    write_replica_sequence(root, W, H, N_FRAMES)
    parser = Parser("Replica", "room0", normalize=False, device="cpu", input_folder=str(root))
    frames = [parser.frame(i) for i in range(N_FRAMES)]
    return root, frames


def _fields(d):
    return {k: getattr(d, k) for k in d.__dataclass_fields__}


def test_pair_placed_with_a_given_pose(sequence):
    root, frames = sequence
    parser = Parser("Replica", "room0", normalize=False, device="cpu", input_folder=str(root))
    i = 2
    want, got = _fields(parser[i]), _fields(parser.pair(i, tar_c2w=frames[i][2]))
    assert set(want) == set(got) and "norm_T" in want and want["norm_T"] is None and got["norm_T"] is None
    for k, v in want.items():
        if torch.is_tensor(v):
            assert torch.equal(v, got[k]), k  # bit for bit
        else:
            assert v == got[k], k
    assert _fields(parser.pair(i)).keys() == want.keys() and torch.equal(parser.pair(i).tar_points, want["tar_points"])
    # another pose: both clouds are placed with it, the read-out pose stays the ground truth of frame i + 1
    P = _pose((0.2, -0.5, 0.8), 33.0, (0.3, 0.1, -0.2))
    d = parser.pair(i, tar_c2w=P)
    K = parser.K
    for pts, depth in ((d.tar_points, frames[i][0]), (d.src_points, frames[i + 1][0])):
        cam = depth_to_points(depth, K)
        assert torch.allclose(pts, cam @ P[:3, :3].T + P[:3, 3], atol=1e-6)
    assert torch.equal(d.tar_c2w, P) and torch.equal(d.src_c2w, frames[i + 1][2])
    assert torch.equal(d.src_depth.reshape(H, W), frames[i + 1][0])


class _PerfectTracker:
    """Stands in for GraphTracker: run() returns the reference pose load_frame was given -- the exact ground truth of the
    new frame, expressed in the pair's frame -- as the minimum-loss pose."""
    made = []

    def __init__(self, N, W_, H_, config, device, render_mode):
        self.args = (N, W_, H_, render_mode)
        self.loads = []
        _PerfectTracker.made.append(self)

    def load_frame(self, tar_points, colors, scales, src_depth, tar_c2w, src_c2w, K, pixels=None):
        assert tar_points.shape == (self.args[0], 3) and scales.shape == tar_points.shape
        assert src_depth.reshape(-1).shape[0] == W * H
        self.loads.append(dict(init=tar_c2w.clone(), gt=src_c2w.clone(), pixels=pixels, tar_points=tar_points.clone()))

    def run(self):
        gt = self.loads[-1]["gt"]
        return TrackResult(best_loss=0.25, steps=12, final_c2w=torch.eye(4), best_c2w=gt.clone(), best_step=7)


@pytest.mark.parametrize("motion,normalize", [("hold", True), ("constant_velocity", True), ("hold", False),
                                              ("constant_velocity", False)])
def test_localizer_composition_with_a_perfect_tracker(sequence, motion, normalize, monkeypatch):
    """6 tracked frames: with a tracker that answers the exact pose in the pair's frame the trajectory is the ground
    truth within 1e-5 -- a wrong multiplication order or a missing de-normalisation leaves errors of the size of the
    poses themselves.  (With normalize the query depth is re-rendered on the GPU; the stand-in tracker does not look at
    it, so that render is replaced here.)"""
    import gsplatloc_amd.data.dataset as DS

    monkeypatch.setattr(DS, "compute_depth_gt", lambda pts, col, Ks, c2w, height, width: torch.zeros(height, width))
    _, frames = sequence
    _PerfectTracker.made = []
    loc = Localizer(replica_intrinsics(W, H), W, H, TrackerConfig(max_steps=5), normalize=normalize, motion=motion,
                    device="cpu", tracker_factory=_PerfectTracker)
    with pytest.raises(RuntimeError, match="reset"):
        loc.track(frames[1][0])
    loc.reset(frames[0][0], frames[0][1], frames[0][2])
    results = [loc.track(d, rgb, gt_c2w=pose) for d, rgb, pose in frames[1:]]
    traj = loc.trajectory
    gt = torch.stack([f[2] for f in frames])
    assert traj.shape == (N_FRAMES, 4, 4)
    assert float((traj - gt).abs().max()) <= 1e-5, (traj - gt).abs().amax(dim=(1, 2))
    assert len(_PerfectTracker.made) == 1 and _PerfectTracker.made[0].args == (W * H, W, H, "ED")  # one tracker kept
    loads = _PerfectTracker.made[0].loads
    for k, r in enumerate(results, start=1):
        assert isinstance(r, LocalizeResult) and not r.lost and r.best_step == 7 and r.steps == 12
        assert r.best_loss == 0.25 and r.eT <= 1e-5 and r.eR <= 1e-3
        # the start: the previous estimate, or from the third frame on the constant-velocity prediction
        if motion == "hold" or k == 1:
            want_init = traj[k - 1]
        else:
            want_init = predict_pose(traj[k - 2], traj[k - 1])
        assert torch.allclose(r.init_c2w, want_init, atol=1e-6)
        # ... handed to the tracker in the pair's frame: brought back, it is the same pose
        if normalize:
            T = align_principle_axes(depth_to_points(frames[k - 1][0], loc.K) @ traj[k - 1][:3, :3].T + traj[k - 1][:3, 3])
            assert torch.allclose(denormalize_camera(T, loads[k - 1]["init"]), want_init, atol=2e-6)
        else:
            assert torch.equal(loads[k - 1]["init"], want_init)
        assert loads[k - 1]["pixels"] is None


class _LostTracker(_PerfectTracker):
    def run(self):
        gt = self.loads[-1]["gt"]
        return TrackResult(steps=5, final_c2w=gt.clone(), best_c2w=gt.clone(), best_step=-1)


def test_localizer_reports_a_lost_frame(sequence):
    """No minimum was recorded (best_step == -1): the frame is flagged, its pose is the last iterate's."""
    _, frames = sequence
    loc = Localizer(replica_intrinsics(W, H), W, H, TrackerConfig(max_steps=5), normalize=False, device="cpu",
                    tracker_factory=_LostTracker)
    loc.reset(frames[0][0])  # no image, identity pose
    assert torch.equal(loc.trajectory, torch.eye(4)[None])
    r = loc.track(frames[1][0])
    assert r.lost and r.best_step == -1 and r.eT is None and r.eR is None and loc.trajectory.shape == (2, 4, 4)


def test_localizer_photometric_term_needs_the_image(sequence):
    _, frames = sequence
    _PerfectTracker.made = []
    loc = Localizer(replica_intrinsics(W, H), W, H, TrackerConfig(max_steps=5, rgb_lambda=0.2), normalize=False,
                    motion="hold", device="cpu", tracker_factory=_PerfectTracker)
    with pytest.raises(ValueError, match="rgb"):
        loc.reset(frames[0][0], None, frames[0][2])
    loc.reset(frames[0][0], frames[0][1], frames[0][2])
    with pytest.raises(ValueError, match="rgb"):
        loc.track(frames[1][0], None)
    loc.track(frames[1][0], frames[1][1])
    made = _PerfectTracker.made[0]
    assert made.args[3] == "RGB+ED" and made.loads[0]["pixels"].shape == (1, H, W, 3)
    with pytest.raises(ValueError, match="motion"):
        Localizer(replica_intrinsics(W, H), W, H, motion="spline", device="cpu")


def test_pose_step_best_rejects_a_null_best_pose():
    """gsl_pose_step_best with best_pose = NULL: GSL_ERR_BAD_ARG (-1), decided on the host before any launch."""
    from gsplatloc_amd._lib import load_library, ptr

    lib = load_library()
    pose_f, pose_i = torch.zeros(40), torch.zeros(4, dtype=torch.int32)
    c2w, viewmat, eye = torch.eye(4), torch.eye(4), torch.eye(4)
    hist, v_viewmat, sums, best = torch.zeros(10), torch.zeros(16), torch.ones(3), torch.zeros(24)

    def call(best_pose, photo=None):
        return lib.gsl_pose_step_best(ptr(pose_f), ptr(pose_i), ptr(v_viewmat), None, 0, None, None, 0, ptr(sums), None,
                                      ptr(eye), 64, 48, 0.8, 0.2, 0.0, 0.9, 0.999, 1e-8, 1e-3, 1e-3, 0.99, 100, 200, 1, 10,
                                      ptr(c2w), ptr(viewmat), ptr(hist), None, ptr(photo), 0.0, 0.0, ptr(best_pose))

    assert call(None) == -1
    assert call(None, photo=torch.ones(3)) == -1
    if not torch.cuda.is_available():  # host pointers: with every argument in place the launch itself is refused
        assert call(best) == -3
    assert math.isfinite(float(best.sum())) and not best.any()  # nothing wrote to it
