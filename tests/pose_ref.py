"""Dataset-scale poses and the reference's pose loop without a render (shared by the pose-step and far-pose tests).

``far_poses()``: camera-to-world matrices as the product sees them after ``data/normalize.py:normalize_pair`` -- an
arbitrary rotation, mostly with a negative trace, and a translation of metres -- one per branch of the
rotation-matrix-to-quaternion conversion.

``reference_pose_loop()``: the loop of ``oracle.tracker_oracle.track_frame`` with the render replaced by given inputs:
the loss is handed in as its sums and the gradient of the view matrix as a matrix, so that the pose chain, the two Adam
optimisers, the learning-rate decay, the pose errors and the early-stop bookkeeping can be compared step by step.  Run
in float64 it is the truth; run in float32 its distance from the float64 run is the floor of any float32 comparison.
"""
import math
from dataclasses import dataclass

import torch

from oracle import tracker_oracle as T

FAR_TRANSLATION = (3.2, -1.7, 0.9)
# name -> (axis, degrees, branch of rotation_matrix_to_quaternion)
FAR_CASES = {
    "trace>0": ((0.3, -0.8, 0.5), 75.0, "c0"),
    "m00": ((1.0, 0.15, -0.1), 170.0, "c1"),
    "m11": ((0.1, 1.0, 0.2), 165.0, "c2"),
    "m22": ((-0.15, 0.1, 1.0), 175.0, "c3"),
    "pi_exact": ((0.0, 0.0, 1.0), 180.0, "c3"),
}


def axis_angle(axis, deg):
    """float64 rotation about ``axis`` by ``deg`` degrees (Rodrigues); multiples of 90 degrees come out exact."""
    ax = torch.tensor(axis, dtype=torch.float64)
    ax = ax / ax.norm()
    q, r = divmod(deg, 90.0)
    if r == 0.0:
        s, c = ((0.0, 1.0), (1.0, 0.0), (0.0, -1.0), (-1.0, 0.0))[int(q) % 4]
    else:
        s, c = math.sin(math.radians(deg)), math.cos(math.radians(deg))
    Kx = torch.tensor([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]], dtype=torch.float64)
    return torch.eye(3, dtype=torch.float64) + s * Kx + (1 - c) * (Kx @ Kx)


def far_poses():
    """name -> c2w [4,4] float64."""
    out = {}
    for name, (axis, deg, _) in FAR_CASES.items():
        c2w = torch.eye(4, dtype=torch.float64)
        c2w[:3, :3] = axis_angle(axis, deg)
        c2w[:3, 3] = torch.tensor(FAR_TRANSLATION, dtype=torch.float64)
        out[name] = c2w
    return out


def branch(R):
    """The branch of ``rotation_matrix_to_quaternion`` that ``R`` takes (its conditions restated: the oracle has no flag)."""
    m00, m11, m22 = float(R[0, 0]), float(R[1, 1]), float(R[2, 2])
    if m00 + m11 + m22 > 0.0:
        return "c0"
    if m00 > m11 and m00 > m22:
        return "c1"
    return "c2" if m11 > m22 else "c3"


@dataclass
class PoseHyper:
    """What gsl_pose_init / gsl_pose_step take (defaults: the reference's rates, betas and epsilon)."""
    quat_lr: float = 5e-4
    trans_lr: float = 1e-3
    wd_quat: float = 1e-3
    wd_trans: float = 1e-3
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = 1e-8
    gamma: float = 0.2 ** (1.0 / 25)
    min_step: int = 2
    patience: int = 1000
    early_stop: bool = True
    max_steps: int = 25
    width: int = 16
    height: int = 16
    depth_w: float = 0.8
    edge_w: float = 0.2
    normal_w: float = 0.0


def reference_pose_loop(dtype, init_c2w, gt_c2w, v_viewmats, loss_sums, hyper, q_scale=1.0):
    """One record per row of ``v_viewmats`` [n,16] / ``loss_sums`` [n,3] (sum |depth error|, sum |edge error|, sum of
    row cosines): the state AFTER that call of the loop body, as float64 tensors and ints.  Once the loop has stopped
    (patience, or ``max_steps`` -- which track_frame leaves to its ``range``) further calls repeat the last record.
    ``q_scale`` scales the initial quaternion (the parametrisation normalises it)."""
    hp = hyper
    init_c2w, gt_c2w = init_c2w.to(dtype), gt_c2w.to(dtype)
    q = torch.nn.Parameter(T.rotation_matrix_to_quaternion(init_c2w[:3, :3].contiguous()) * q_scale)
    t = torch.nn.Parameter(init_c2w[:3, 3].clone())
    opt_q = torch.optim.Adam([q], lr=hp.quat_lr, betas=(hp.beta1, hp.beta2), eps=hp.eps, weight_decay=hp.wd_quat)
    opt_t = torch.optim.Adam([t], lr=hp.trans_lr, betas=(hp.beta1, hp.beta2), eps=hp.eps, weight_decay=hp.wd_trans)
    sch = [torch.optim.lr_scheduler.ExponentialLR(o, gamma=hp.gamma) for o in (opt_q, opt_t)]
    inf = float("inf")
    best = dict(best_loss=inf, best_eT=inf, best_eR=inf, best_step=-1)
    counter, stopped, step = 0, 0, 0
    zeros7 = torch.zeros(7, dtype=torch.float64)
    m, v = zeros7.clone(), zeros7.clone()
    records = []
    inv_P = 1.0 / (hp.width * hp.height)
    for k in range(v_viewmats.shape[0]):
        if stopped:
            records.append(dict(records[-1]))
            continue
        opt_q.zero_grad(set_to_none=True)
        opt_t.zero_grad(set_to_none=True)
        c2w = T.camera_forward(q, t)
        V = torch.linalg.inv(c2w)
        (V[:3] * v_viewmats[k].to(dtype).reshape(4, 4)[:3]).sum().backward()
        s = loss_sums[k].to(dtype)
        total = hp.depth_w * (s[0] * inv_P) + hp.edge_w * (s[1] * inv_P)
        if hp.normal_w != 0.0:
            total = total + hp.normal_w * (1.0 - s[2] * (1.0 / (3.0 * hp.height)))
        lv = float(total)
        eT = T.calculate_translation_error(c2w.detach(), gt_c2w)
        eR = T.calculate_rotation_error(c2w.detach(), gt_c2w)
        if hp.early_stop and step > hp.min_step:
            if lv < best["best_loss"]:
                best = dict(best_loss=lv, best_eT=eT, best_eR=eR, best_step=step)
                counter = 0
            else:
                counter += 1
        grad_q, grad_t = q.grad.detach().double().clone(), t.grad.detach().double().clone()
        step += 1
        if hp.early_stop and counter >= hp.patience:
            stopped = 1  # the break before the optimiser step
        else:
            if step >= hp.max_steps:
                stopped = 1  # the last iteration still takes its step
            opt_q.step()
            opt_t.step()
            for sc in sch:
                sc.step()
            m = torch.cat([opt_q.state[q]["exp_avg"], opt_t.state[t]["exp_avg"]]).detach().double().clone()
            v = torch.cat([opt_q.state[q]["exp_avg_sq"], opt_t.state[t]["exp_avg_sq"]]).detach().double().clone()
        with torch.no_grad():
            # the pose to render next; once stopped, the final pose: the last one rendered (track_frame's final_c2w)
            c2w_new = c2w.detach() if stopped else T.camera_forward(q, t)
            rec = dict(q=q.detach().double().clone(), t=t.detach().double().clone(), grad_q=grad_q, grad_t=grad_t, m=m, v=v,
                       lr=torch.tensor([opt_q.param_groups[0]["lr"], opt_t.param_groups[0]["lr"]], dtype=torch.float64),
                       c2w=c2w_new.double(), viewmat=torch.linalg.inv(c2w_new).double(),
                       loss=torch.tensor(lv, dtype=torch.float64), eT=torch.tensor(eT, dtype=torch.float64),
                       eR=torch.tensor(eR, dtype=torch.float64), step=step, counter=counter, stopped=stopped)
        rec.update({kk: (vv if kk == "best_step" else torch.tensor(vv, dtype=torch.float64)) for kk, vv in best.items()})
        records.append(rec)
    return records


def random_v_viewmats(n, seed):
    """[n,16] float64 holding float32 values of magnitude 10^N(0,1) and random sign; row 3 is non-zero garbage that a
    consumer must ignore (that row of a view matrix is constant)."""
    g = torch.Generator().manual_seed(seed)
    mag = 10.0 ** torch.randn(n, 16, generator=g, dtype=torch.float64)
    sign = torch.where(torch.rand(n, 16, generator=g) < 0.5, -1.0, 1.0).double()
    return (mag * sign).float().double()


def random_loss_sums(n, seed, pixels):
    """[n,3] float64 holding float32 values: two positive loss sums of the order of the pixel count, one cosine sum."""
    g = torch.Generator().manual_seed(seed)
    s = torch.rand(n, 3, generator=g, dtype=torch.float64)
    s[:, :2] = s[:, :2] * 0.1 * pixels + 1e-3 * pixels
    return s.float().double()
