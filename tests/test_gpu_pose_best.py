"""gsl_pose_step_best: the pose step that also keeps the minimum-loss POSE (best_pose[24]), as a unit.

No render: 12 calls through the C ABI on hand-made device buffers (gradients and loss sums of tests/pose_ref.py), min_step
= 2 so that calls 3..11 are eligible.  The loss sums are rescaled so that the totals -- computed here in float64 from the
float32 values the device is given -- follow a designed curve: every total differs from every other by 2 % or more (the
issue asks for 1e-3 relative), new minima at calls 3, 4, 5 and 6, the first (and only) global minimum at call 6, a second
dip at call 9 that stays above it.  Call 6 is neither the first eligible call nor the last.

Asserted: best_pose is untouched (a sentinel) until the first eligible call; after every call it holds, bit for bit, the
quaternion, translation (pose_f[0:7]) and camera-to-world matrix (c2w) snapshotted BEFORE the call that set the running
minimum, and that call's total (== pose_f[23]); pose_i[3] is that call's step.  The same inputs through gsl_pose_step
(and, with photo_sums, through gsl_pose_step_photo) leave pose_f, pose_i, c2w, viewmat and loss_hist bit-identical
after every call."""
import pytest
import torch

from tests.pose_ref import PoseHyper, far_poses, random_loss_sums, random_v_viewmats

pytestmark = pytest.mark.gpu

DEV = "cuda"
N_CALLS = 12
TARGETS = (1.0, 0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.45, 0.52, 0.42, 0.55, 0.62)
MIN_CALL = 6
SENTINEL = -123.25
RGB_W, SSIM_W = 0.2, 0.5


def _photo_term(ps, hp):
    """The photometric term as csrc/tracker.hip forms it from (sum m, sum |c - p|, sum S), float64."""
    n_windows = 3.0 * (hp.width - 10) * (hp.height - 10)
    l1 = ps[:, 1] / (ps[:, 0] + 1e-8)
    return RGB_W * ((1.0 - SSIM_W) * l1 + SSIM_W * (1.0 - ps[:, 2] / n_windows))


def _inputs(hp, photo):
    """(v_viewmat [12,16], loss_sums [12,3], photo_sums [12,3] or None) as float64 tensors of float32 values, and the
    totals the device will compute (float64 on the host)."""
    P = hp.width * hp.height
    vv = random_v_viewmats(N_CALLS, seed=21)
    ls = random_loss_sums(N_CALLS, seed=22, pixels=P)
    ps, extra = None, torch.zeros(N_CALLS, dtype=torch.float64)
    if photo:
        g = torch.Generator().manual_seed(23)
        r = torch.rand(N_CALLS, 3, generator=g, dtype=torch.float64)
        ps = torch.stack([200.0 + 20.0 * r[:, 0], 20.0 + 20.0 * r[:, 1], 50.0 + 50.0 * r[:, 2]], 1).float().double()
        extra = _photo_term(ps, hp)
    dw, ew = float(torch.tensor(hp.depth_w).float()), float(torch.tensor(hp.edge_w).float())
    base = (dw * ls[:, 0] + ew * ls[:, 1]) / P
    want = torch.tensor(TARGETS, dtype=torch.float64) - extra
    assert bool((want > 0).all())
    ls[:, :2] = (ls[:, :2] * (want / base)[:, None]).float().double()
    totals = (dw * ls[:, 0] + ew * ls[:, 1]) / P + extra
    # the design, checked on the numbers the device gets
    rel = (totals[:, None] - totals[None, :]).abs() / torch.maximum(totals[:, None], totals[None, :]) + torch.eye(N_CALLS)
    assert float(rel.min()) >= 1e-3
    eligible = totals[hp.min_step + 1:]
    assert int(eligible.argmin()) + hp.min_step + 1 == MIN_CALL and hp.min_step + 1 < MIN_CALL < N_CALLS - 1
    return vv, ls, ps, totals


class _Tail:
    """One tracker's pose buffers; step() through the entry point named."""

    def __init__(self, hp, init, gt):
        from gsplatloc_amd._lib import check, current_stream, load_library, ptr
        self.lib, self.hp = load_library(), hp
        self.pose_f = torch.full((40,), 7.5, device=DEV)
        self.pose_i = torch.full((4,), 9, dtype=torch.int32, device=DEV)
        self.c2w = torch.full((16,), 7.5, device=DEV)
        self.viewmat = torch.full((16,), 7.5, device=DEV)
        self.hist = torch.full((32,), -1.0, device=DEV)
        self.best = torch.full((24,), SENTINEL, device=DEV)
        self.gt = gt.float().contiguous().to(DEV)
        self.init_c2w = init.float().contiguous().to(DEV)
        check(self.lib.gsl_pose_init(ptr(self.pose_f), ptr(self.pose_i), ptr(self.init_c2w), hp.quat_lr, hp.trans_lr,
                                     ptr(self.c2w), ptr(self.viewmat), current_stream()), "gsl_pose_init")
        self.pose_f[34:36] = float("inf")

    def step(self, entry, v_viewmat, loss_sums, photo_sums=None):
        from gsplatloc_amd._lib import check, current_stream, ptr
        hp = self.hp
        args = (ptr(self.pose_f), ptr(self.pose_i), ptr(v_viewmat), None, 0, None, None, 0, ptr(loss_sums), None,
                ptr(self.gt), hp.width, hp.height, hp.depth_w, hp.edge_w, hp.normal_w, hp.beta1, hp.beta2, hp.eps,
                hp.wd_quat, hp.wd_trans, hp.gamma, hp.min_step, hp.patience, int(hp.early_stop), hp.max_steps,
                ptr(self.c2w), ptr(self.viewmat), ptr(self.hist), current_stream())
        photo = (ptr(photo_sums), RGB_W if photo_sums is not None else 0.0, SSIM_W if photo_sums is not None else 0.0)
        if entry == "gsl_pose_step_best":
            check(self.lib.gsl_pose_step_best(*args, *photo, ptr(self.best)), entry)
        elif entry == "gsl_pose_step_photo":
            check(self.lib.gsl_pose_step_photo(*args, *photo), entry)
        else:
            assert photo_sums is None
            check(self.lib.gsl_pose_step(*args), entry)

    def state(self):
        torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().clone() for k in ("pose_f", "pose_i", "c2w", "viewmat", "hist", "best")}


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("photo", [False, True], ids=["depth", "photo"])
def test_best_pose_is_the_minimum_loss_iterate_and_nothing_else_moves(photo):
    hp = PoseHyper(min_step=2, patience=1000, max_steps=25)
    poses = far_poses()
    init, gt = poses["m00"], poses["trace>0"]  # dataset-scale: a rotation of 170 degrees, metres of translation
    vv, ls, ps, totals = _inputs(hp, photo)
    vv_d, ls_d = vv.float().to(DEV), ls.float().to(DEV)
    ps_d = ps.float().to(DEV) if photo else None
    new, old = _Tail(hp, init, gt), _Tail(hp, init, gt)
    old_entry = "gsl_pose_step_photo" if photo else "gsl_pose_step"
    running, snap_at_best = None, None
    for k in range(N_CALLS):
        before = new.state()
        new.step("gsl_pose_step_best", vv_d[k], ls_d[k], ps_d[k] if photo else None)
        old.step(old_entry, vv_d[k], ls_d[k], ps_d[k] if photo else None)
        a, b = new.state(), old.state()
        for key in ("pose_f", "pose_i", "c2w", "viewmat", "hist"):
            assert torch.equal(_bits(a[key]), _bits(b[key])), (k, key, a[key], b[key])
        assert bool((b["best"] == SENTINEL).all())  # the other entry points never see the buffer
        assert int(a["pose_i"][0]) == k + 1
        if k > hp.min_step and (running is None or float(totals[k]) < running):
            running, snap_at_best, best_call = float(totals[k]), before, k
        if snap_at_best is None:
            assert bool((a["best"] == SENTINEL).all()), (k, a["best"])
            assert int(a["pose_i"][3]) == -1
            continue
        assert int(a["pose_i"][3]) == best_call, (k, a["pose_i"])
        assert torch.equal(_bits(a["best"][0:7]), _bits(snap_at_best["pose_f"][0:7])), (k, a["best"], snap_at_best["pose_f"])
        assert torch.equal(_bits(a["best"][8:24]), _bits(snap_at_best["c2w"])), (k, a["best"][8:24], snap_at_best["c2w"])
        assert torch.equal(_bits(a["best"][7:8]), _bits(a["pose_f"][23:24]))
        assert abs(float(a["best"][7]) - running) <= 1e-6 * running, (k, float(a["best"][7]), running)
    assert best_call == MIN_CALL and int(a["pose_i"][3]) == MIN_CALL
    # the pose kept is the one BEFORE that call's Adam update, not the one it led to
    assert not torch.equal(a["best"][0:7], a["pose_f"][0:7])
