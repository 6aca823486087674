"""The tracker's tail -- gsl_pose_init, gsl_pose_step, gsl_pack_pose_reduce -- as a unit, at dataset-scale poses.

No render: the kernels are driven through the C ABI on hand-made device buffers and compared, call by call, with
tests/pose_ref.py:reference_pose_loop (the reference's loop with the render replaced by the same inputs).

Comparison rule for every float quantity:   |device - float64 reference|  <=  max(4 x floor, one float32 ulp of the
quantity's magnitude),   floor = |float32 reference - float64 reference| on the same case.  The factor 4 covers a
different but equally valid operation order in the ~600 dependent float32 operations of a step.  Every quantity is
compared after every call; a trajectory is one case, so the largest device error over its calls is held against the
largest float32-reference error over its calls.  The floor of a single call is one draw of rounding noise -- the
float32 reference lands within a quarter ulp of the float64 one at some calls by chance, where no float32 state that
has been rounded a dozen times can follow -- so the single-call form of the rule is evaluated and printed (how many
comparisons, how many beyond 4 x their own call's floor, the worst ratio) but not asserted.  Every test prints, per
quantity, its largest device error with the floor of that case and the largest error in units of
max(floor, ulp / 4) (the rule allows 4), through tests.parity.report.
"""
import math

import pytest
import torch

from oracle import tracker_oracle as T
from tests.parity import report
from tests.pose_ref import (PoseHyper, axis_angle, far_poses, random_loss_sums, random_v_viewmats, reference_pose_loop)
from tests.scenes import small_pose

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS32 = float(torch.finfo(torch.float32).eps)
# pose_f slices (layout: csrc/tracker.hip)
SL = dict(q=slice(0, 4), t=slice(4, 7), m=slice(7, 14), v=slice(14, 21), lr=slice(21, 23), best_loss=23, best_eT=26,
          best_eR=27, loss=28, eT=29, eR=30)
STEP_FIELDS = ("q", "t", "m", "v", "lr", "c2w", "viewmat", "loss", "eT")
BEST_FIELDS = ("best_loss", "best_eT", "best_eR")


def _f32(x):
    """float64 tensor holding float32 values: what the device is given is what the references start from."""
    return x.float().double()


class Rule:
    """The comparison rule, per quantity and case.  A case is what the floor is measured on: one trajectory (all its
    calls together: the largest device error against the largest float32-reference error of the quantity), one partial
    count, one row count.  Everything is asserted at the end so that a failing run still prints every figure."""

    def __init__(self, tag):
        self.tag, self.acc, self.failures = tag, {}, []
        self.calls, self.call_misses, self.call_worst = 0, 0, 0.0

    def add(self, name, dev, r64, r32, case="", where=""):
        dev, r64, r32 = (torch.as_tensor(x).detach().double().cpu().reshape(-1) for x in (dev, r64, r32))
        fin = torch.isfinite(r64)
        if not bool(fin.all()):  # +inf before the first best: exactly that
            if not torch.equal(dev[~fin], r64[~fin]):
                self.failures.append((name, case, where, "non-finite entries differ", dev.tolist(), r64.tolist()))
            dev, r64, r32 = dev[fin], r64[fin], r32[fin]
            if dev.numel() == 0:
                return
        if not bool(torch.isfinite(dev).all()):
            self.failures.append((name, case, where, "device value not finite", dev.tolist()))
            return
        err, floor = float((dev - r64).abs().max()), float((r32 - r64).abs().max())
        # recorded, not asserted: the same rule with the floor of this single call (see the module docstring)
        ulp = EPS32 * float(r64.abs().max())
        self.calls += 1
        self.call_misses += err > max(4.0 * floor, ulp)
        if err > 0.0:
            self.call_worst = max(self.call_worst, err / max(floor, ulp / 4.0))
        e0, f0, m0 = self.acc.get((name, case), (0.0, 0.0, 0.0))
        self.acc[(name, case)] = (max(e0, err), max(f0, floor), max(m0, float(r64.abs().max())))

    def finish(self):
        figs, worst = {}, {}
        for (name, case), (err, floor, mag) in self.acc.items():
            ulp = EPS32 * mag
            ratio = err / max(floor, ulp / 4.0) if err > 0.0 else 0.0
            if name not in worst or ratio > worst[name][2]:
                worst[name] = (err, floor, ratio)
            if err > max(4.0 * floor, ulp):
                self.failures.append((name, case, f"err {err:.3e} > max(4 x floor {floor:.3e}, ulp {ulp:.3e})"))
        for name, (err, floor, ratio) in worst.items():
            figs[name + " err"] = err
            figs[name + " floor"] = floor
        figs["worst err/floor (allowed 4)"] = max((w[2] for w in worst.values()), default=0.0)
        figs["single-call comparisons"] = self.calls
        figs["of them beyond their own call's floor x 4"] = self.call_misses
        figs["worst single-call err/floor"] = self.call_worst
        report(self.tag, 0.0, **figs)
        assert not self.failures, (self.tag, self.failures)


class Device:
    """The buffers of one tracker and the two calls."""

    def __init__(self, hp, gt_c2w, n_hist=64):
        from gsplatloc_amd._lib import load_library
        self.lib, self.hp = load_library(), hp
        self.pose_f = torch.full((40,), 7.5, device=DEV)  # garbage that init has to replace
        self.pose_i = torch.full((4,), 9, dtype=torch.int32, device=DEV)
        self.c2w = torch.full((16,), 7.5, device=DEV)
        self.viewmat = torch.full((16,), 7.5, device=DEV)
        self.hist = torch.full((n_hist,), -1.0, device=DEV)
        self.gt = gt_c2w.float().contiguous().to(DEV)

    def init(self, c2w):
        from gsplatloc_amd._lib import check, current_stream, ptr
        self.init_c2w = c2w.float().contiguous().to(DEV)
        check(self.lib.gsl_pose_init(ptr(self.pose_f), ptr(self.pose_i), ptr(self.init_c2w), self.hp.quat_lr,
                                     self.hp.trans_lr, ptr(self.c2w), ptr(self.viewmat), current_stream()), "gsl_pose_init")
        return self

    def step(self, v_viewmat=None, rows=None, n_rows=0, K=None, partials=None, n_partials=0, loss_sums=None,
             normal_sum=None):
        from gsplatloc_amd._lib import check, current_stream, ptr
        hp = self.hp
        check(self.lib.gsl_pose_step(ptr(self.pose_f), ptr(self.pose_i), ptr(v_viewmat), ptr(rows), n_rows, ptr(K),
                                     ptr(partials), n_partials, ptr(loss_sums), ptr(normal_sum), ptr(self.gt), hp.width,
                                     hp.height, hp.depth_w, hp.edge_w, hp.normal_w, hp.beta1, hp.beta2, hp.eps,
                                     hp.wd_quat, hp.wd_trans, hp.gamma, hp.min_step, hp.patience, int(hp.early_stop),
                                     hp.max_steps, ptr(self.c2w), ptr(self.viewmat), ptr(self.hist), current_stream()),
              "gsl_pose_step")

    def state(self):
        torch.cuda.synchronize()
        return dict(f=self.pose_f.cpu().clone(), i=self.pose_i.cpu().clone(), c2w=self.c2w.cpu().clone(),
                    viewmat=self.viewmat.cpu().clone(), hist=self.hist.cpu().clone())


def _same_bits(a, b, keys=("f", "i", "c2w", "viewmat", "hist")):
    return [k for k in keys if not torch.equal(a[k].view(torch.int32), b[k].view(torch.int32))]


def _dev_field(st, name):
    if name in ("c2w", "viewmat"):
        return st[name].reshape(4, 4)
    return st["f"][SL[name]]


def _compare_call(rule, st, r64, r32, k, fields):
    for name in fields:
        rule.add(name, _dev_field(st, name), r64[name], r32[name], where=f"call {k}")
    got = tuple(st["i"].tolist())
    want = (r64["step"], r64["counter"], r64["stopped"], r64["best_step"])
    if got != want:
        rule.failures.append(("pose_i", f"call {k}", got, want))


def _run_trajectory(tag, init, gt, vv, ls, hp, q_scale=1.0, fields=STEP_FIELDS + BEST_FIELDS):
    """Device and both references over len(vv) calls; returns the device states."""
    init, gt = _f32(init), _f32(gt)
    r64 = reference_pose_loop(torch.float64, init, gt, vv, ls, hp, q_scale=q_scale)
    r32 = reference_pose_loop(torch.float32, init, gt, vv, ls, hp, q_scale=q_scale)
    dev = Device(hp, gt).init(init)
    if q_scale != 1.0:
        dev.pose_f[0:4] *= q_scale
    vv_d, ls_d = vv.float().to(DEV), ls.float().to(DEV)
    rule, states = Rule(tag), []
    for k in range(vv.shape[0]):
        before = r64[k - 1]["step"] if k else 0
        dev.step(v_viewmat=vv_d[k], loss_sums=ls_d[k])
        st = dev.state()
        states.append(st)
        _compare_call(rule, st, r64[k], r32[k], k, fields)
        if r64[k]["step"] > before:  # this call was an iteration: its loss is in the history, later entries untouched
            rule.add("loss_hist", st["hist"][before], r64[k]["loss"], r32[k]["loss"], where=f"call {k}")
            if not bool((st["hist"][before + 1:] == -1.0).all()):
                rule.failures.append(("loss_hist", f"call {k}", "entries past the step were written"))
    rule.finish()
    return states, r64


POSES = far_poses()


# ------------------------------------------------------------------------------------------------------------ a. init
@pytest.mark.parametrize("name", list(POSES) + ["identity"])
def test_pose_init_at_far_poses(name):
    init = _f32(POSES[name]) if name != "identity" else torch.eye(4, dtype=torch.float64)
    hp = PoseHyper()
    dev = Device(hp, init).init(init)
    st = dev.state()
    f = st["f"]
    ref = {}
    for dt in (torch.float64, torch.float32):
        q = T.rotation_matrix_to_quaternion(init.to(dt)[:3, :3].contiguous())
        c2w = T.camera_forward(q, init.to(dt)[:3, 3])
        ref[dt] = dict(q=q, t=init.to(dt)[:3, 3], c2w=c2w, viewmat=torch.linalg.inv(c2w))
    rule = Rule(f"pose init {name}")
    for k in ("q", "t", "c2w", "viewmat"):
        rule.add(k, _dev_field(st, k), ref[torch.float64][k], ref[torch.float32][k])
    assert torch.equal(f[4:7], init[:3, 3].float())
    assert torch.equal(f[7:21], torch.zeros(14))
    assert torch.equal(f[21:23], torch.tensor([hp.quat_lr, hp.trans_lr], dtype=torch.float32))
    assert bool((f[23:31] == float("inf")).all())
    assert st["i"].tolist() == [0, 0, 0, -1]
    assert torch.equal(st["c2w"][12:], torch.tensor([0.0, 0, 0, 1])) and torch.equal(st["viewmat"][12:], torch.tensor([0.0, 0, 0, 1]))
    if name == "pi_exact":
        q = f[0:4].double()
        assert abs(float(q.norm()) - 1.0) <= EPS32
        assert float((T.quaternion_to_rotation_matrix(q) - init[:3, :3]).abs().max()) <= 2 * EPS32
    rule.finish()


# ------------------------------------------------------------------------------------------------- b. step trajectory
@pytest.mark.parametrize("name", list(POSES))
def test_pose_step_trajectory_at_far_poses(name):
    init = POSES[name]
    n = 25
    hp = PoseHyper()  # wd 1e-3, betas (0.9, 0.999), eps 1e-8, gamma 0.2^(1/25), min_step 2, patience 1000
    vv = random_v_viewmats(n, seed=100 + list(POSES).index(name))
    ls = random_loss_sums(n, seed=7, pixels=hp.width * hp.height)
    states, r64 = _run_trajectory(f"pose step {name}", init, init @ small_pose(0.3, 0.01), vv, ls, hp)
    assert int(states[-1]["i"][0]) == n and int(states[-1]["i"][2]) == 1 and int(states[-2]["i"][2]) == 0
    # the comparison has something to see: the pose moved four orders beyond float32 resolution
    assert float((r64[-1]["t"] - _f32(init)[:3, 3]).norm()) > 1e-3


def test_pose_step_epsilon_term():
    """Adam's epsilon where it matters.  The translation's own gradient is exactly zero in every step (column 3 of
    v_viewmat is zero), so its Adam gradient is the weight decay 1e-3 * t alone: t = (0, 1e-6, 1e-3) gives one
    component exactly zero in every step (0 / (0 + eps): NaN without the term), one at 1e-9 (eps dominates the
    denominator) and one at 1e-6 (eps is its last per cent).  The rotation is far and gets random gradients."""
    init = POSES["m22"].clone()
    init[:3, 3] = torch.tensor([0.0, 1e-6, 1e-3], dtype=torch.float64)
    n, hp = 25, PoseHyper()
    vv = random_v_viewmats(n, seed=21)
    vv[:, 3] = vv[:, 7] = vv[:, 11] = 0.0
    ls = random_loss_sums(n, seed=8, pixels=hp.width * hp.height)
    states, r64 = _run_trajectory("pose step epsilon", init, init @ small_pose(0.3, 0.01), vv, ls, hp)
    assert all(float(st["f"][4]) == 0.0 and float(st["f"][7 + 4]) == 0.0 and float(st["f"][14 + 4]) == 0.0 for st in states)
    g0 = r64[0]["m"][4:7] / (1 - hp.beta1)
    assert float(g0[0]) == 0.0 and 0.9e-9 < float(g0[1]) < 1.1e-9 and 0.9e-6 < float(g0[2]) < 1.1e-6
    # eps = 1e-8 is visible: the first step of the 1e-9 component is lr * g / (|g| + eps) = lr / 11, not lr
    first = float(states[0]["f"][5]) - float(torch.tensor(1e-6).float())
    assert -0.12 * hp.trans_lr < first < -0.07 * hp.trans_lr, first


def test_pose_step_follows_a_non_unit_quaternion():
    """pose_f[0:4] scaled by 1.7 after init: the parametrisation normalises, the gradient is that of q / |q|."""
    init = POSES["m11"]
    n, hp = 25, PoseHyper()
    vv, ls = random_v_viewmats(n, seed=31), random_loss_sums(n, seed=9, pixels=hp.width * hp.height)
    states, r64 = _run_trajectory("pose step non-unit quaternion", init, init @ small_pose(0.3, 0.01), vv, ls, hp,
                                  q_scale=1.7)
    assert abs(float(states[-1]["f"][0:4].double().norm()) - 1.7) < 0.05
    R = states[-1]["c2w"].reshape(4, 4)[:3, :3].double()
    assert float((R @ R.T - torch.eye(3, dtype=torch.float64)).abs().max()) < 4 * EPS32


# --------------------------------------------------------------------------------------------------- c. rotation error
ANGLES = (1e-3, 0.05, 1.0, 10.0, 90.0, 179.9, 180.0)


@pytest.mark.parametrize("name", ["m00", "m22"])
def test_rotation_error_of_the_pose_step(name):
    """last_eR against float64 calculate_rotation_error for gt = R_delta(angle) R_pose.  Everywhere within 0.03 degrees
    = sqrt(2 * 2^-23) rad, the resolution of the reference's own float32 acos form and the conditioning of either
    form next to 180 degrees; up to 10 degrees within 2e-5 degrees + 1e-4 x angle (the Frobenius form exists for
    that range; the absolute part is about six ulp of a rotation-matrix entry)."""
    est = POSES[name]
    hp = PoseHyper()
    vv = random_v_viewmats(1, seed=3).float().to(DEV)
    ls = random_loss_sums(1, seed=3, pixels=256).float().to(DEV)
    figs, failures = {}, []
    for angle in ANGLES:
        gt = est.clone()
        gt[:3, :3] = axis_angle((0.6, -0.3, 0.74), angle) @ est[:3, :3]
        want = T.calculate_rotation_error(est, gt)
        assert abs(want - angle) < 1e-5 + 1e-9 * angle
        dev = Device(hp, gt).init(est)
        dev.step(v_viewmat=vv[0], loss_sums=ls[0])
        got = float(dev.state()["f"][SL["eR"]])
        err = abs(got - want)
        figs[f"{angle:g} deg"] = err
        if not err <= 0.03:
            failures.append((angle, got, want, "0.03 degrees"))
        if angle <= 10.0 and not err <= 2e-5 + 1e-4 * angle:
            # the same formula restated in float32 on the float32 matrices is the floor: 4 x that
            R32 = T.quaternion_to_rotation_matrix(T.rotation_matrix_to_quaternion(est.float()[:3, :3].contiguous()))
            fro = ((R32 - gt.float()[:3, :3]) ** 2).sum()
            floor = abs(float(2.0 * torch.asin(torch.clamp(torch.sqrt(fro * 0.125), max=1.0)) * 57.29577951308232) - want)
            figs[f"{angle:g} deg floor"] = floor
            if not err <= 4 * floor:
                failures.append((angle, got, want, f"2e-5 + 1e-4 x angle, and 4 x the float32 floor {floor:.2e}"))
    report(f"pose step rotation error {name}", 0.0, **figs)
    assert not failures, failures


# ------------------------------------------------------------------------------------------ d. early stop and freezing
STOP_LOSSES = (5.0, 4.0, 3.0, 2.5, 2.6, 2.4, 2.7, 2.8, 2.9, 1.0, 0.9)


def _scripted_sums(hp, n):
    ls = torch.zeros(n, 3, dtype=torch.float64)
    ls[:, 0] = torch.tensor(STOP_LOSSES[:n], dtype=torch.float64) * hp.width * hp.height
    return ls


def test_early_stop_state_machine():
    init = POSES["m00"]
    hp = PoseHyper(min_step=2, patience=3, max_steps=100, depth_w=1.0, edge_w=0.0)
    n = 11  # stops in call 8; calls 9 and 10 arrive after the stop
    states, r64 = _run_trajectory("pose step early stop", init, init @ small_pose(0.3, 0.01), random_v_viewmats(n, 41),
                                  _scripted_sums(hp, n), hp)
    # what the reference loop does with this sequence (tests/test_pose_ref_cpu.py pins it): step > min_step, so index 2
    # does not update the best
    assert [tuple(st["i"].tolist()) for st in states] == [
        (1, 0, 0, -1), (2, 0, 0, -1), (3, 0, 0, -1), (4, 0, 0, 3), (5, 1, 0, 3), (6, 0, 0, 5), (7, 1, 0, 5), (8, 2, 0, 5),
        (9, 3, 1, 5), (9, 3, 1, 5), (9, 3, 1, 5)]
    assert float(states[2]["f"][23]) == float("inf") and float(states[3]["f"][23]) == 2.5
    assert float(states[8]["f"][23]) == float(torch.tensor(2.4).float()) and float(states[8]["f"][28]) == float(torch.tensor(2.9).float())
    # the stopping iteration takes no optimiser step
    moved = slice(0, 23)
    assert torch.equal(states[8]["f"][moved].view(torch.int32), states[7]["f"][moved].view(torch.int32))
    assert not _same_bits(states[8], states[7], ("c2w", "viewmat"))
    assert not torch.equal(states[7]["f"][0:7], states[6]["f"][0:7])
    # and the state is frozen afterwards
    assert not _same_bits(states[9], states[8]) and not _same_bits(states[10], states[8])
    assert float(states[10]["hist"][9]) == -1.0


def test_last_iteration_still_takes_its_step():
    init = POSES["m00"]
    hp = PoseHyper(min_step=2, patience=3, early_stop=False, max_steps=6, depth_w=1.0, edge_w=0.0)
    n = 7
    states, r64 = _run_trajectory("pose step max_steps", init, init @ small_pose(0.3, 0.01), random_v_viewmats(n, 41),
                                  _scripted_sums(hp, n), hp)
    assert [tuple(st["i"].tolist()) for st in states] == [(k + 1, 0, 0, -1) for k in range(5)] + [(6, 0, 1, -1)] * 2
    assert not torch.equal(states[5]["f"][0:7], states[4]["f"][0:7])       # iteration 5 moved the pose
    assert not torch.equal(states[5]["f"][21:23], states[4]["f"][21:23])   # and decayed the rates
    assert not _same_bits(states[5], states[4], ("c2w", "viewmat"))        # the final pose is the last one rendered
    assert not _same_bits(states[6], states[5])                            # a seventh call changes nothing
    assert bool((states[6]["f"][23:28] == float("inf")).all())             # no best without early_stop


# ------------------------------------------------------------------------------------------------------ e. loss assembly
@pytest.mark.parametrize("variant", ["partials", "normal_sum", "loss_sums[2]"])
def test_loss_assembly(variant):
    init = POSES["m11"]
    W, H = 160, 120
    P = W * H
    normal_w = 0.0 if variant == "partials" else 0.05
    hp = PoseHyper(width=W, height=H, depth_w=0.7, edge_w=0.3 - normal_w, normal_w=normal_w)
    g = torch.Generator().manual_seed(77)
    vv = random_v_viewmats(1, seed=5).float().to(DEV)
    rule = Rule(f"pose step loss assembly {variant}")
    for nb in (1, 255, 256, 257, 1000):
        part = (torch.rand(nb, 2, generator=g) * 3.0 * P / nb + 0.01).float()
        cos = (torch.rand(1, generator=g) * 3.0 * H).float()
        dev = Device(hp, init).init(init)
        guard = torch.full((nb + 8, 2), float("nan"), device=DEV)  # NaN behind the last partial: reading past nb shows
        guard[:nb] = part.to(DEV)
        if variant == "loss_sums[2]":
            sums = torch.cat([part.double().sum(0), cos.double()]).float()
            dev.step(v_viewmat=vv[0], loss_sums=sums.to(DEV))
            p64, p32 = sums.double()[:2], sums[:2]
        else:
            nsum = cos.to(DEV) if variant == "normal_sum" else None
            dev.step(v_viewmat=vv[0], partials=guard, n_partials=nb, normal_sum=nsum)
            p64, p32 = part.double().sum(0), part.sum(0)
        want = {}
        for dt, s in ((torch.float64, p64), (torch.float32, p32)):
            inv_P = torch.tensor(1.0 / P, dtype=dt)
            tot = hp.depth_w * (s[0] * inv_P) + hp.edge_w * (s[1] * inv_P)
            if normal_w:
                tot = tot + normal_w * (1.0 - cos.to(dt)[0] * torch.tensor(1.0 / (3.0 * H), dtype=dt))
            want[dt] = tot
        st = dev.state()
        rule.add("last_loss", st["f"][SL["loss"]], want[torch.float64], want[torch.float32], case=f"nb {nb}")
        assert float(st["hist"][0]) == float(st["f"][SL["loss"]])
    rule.finish()


# ------------------------------------------------------------------------------------------------------ f. row reduction
ROW_COUNTS = (0, 1, 3, 63, 64, 65, 255, 256, 257, 448, 449, 450, 1000, 3907)


def _rows(n, seed):
    """[max(n,1)+4, 16] float32: n random-normal rows (columns 12..14 as large as the rest, so the camera-position chain
    carries weight), column 15 NaN -- row 0's holds the binned mode's state word in production -- and NaN rows behind."""
    g = torch.Generator().manual_seed(seed)
    rows = torch.full((max(n, 1) + 4, 16), float("nan"))
    rows[:n, :15] = torch.randn(n, 15, generator=g)
    return rows


def _chain(tot, V):
    """float64 autograd of <tot_R, R> + <tot_t, t> + <tot_cp, -R^-1 t> with respect to V = [R | t]: [12]."""
    V = V.double().clone().requires_grad_()
    tot = tot.double()
    f = (tot[:9].reshape(3, 3) * V[:3, :3]).sum() + (tot[9:12] * V[:3, 3]).sum() \
        + (tot[12:15] * (-torch.linalg.inv(V[:3, :3]) @ V[:3, 3])).sum()
    f.backward()
    return V.grad[:3].reshape(12).detach()


def _pack(rows, n, V, K, partials, n_part, normal_sum):
    from gsplatloc_amd._lib import check, current_stream, load_library, ptr
    out16 = torch.full((16,), 7.5, device=DEV)
    check(load_library().gsl_pack_pose_reduce(None, ptr(rows), n, ptr(V), ptr(K), ptr(partials), n_part, ptr(normal_sum),
                                              ptr(out16), current_stream()), "gsl_pack_pose_reduce")
    torch.cuda.synchronize()
    return out16


@pytest.mark.parametrize("pose,counts", [("m22", ROW_COUNTS), ("identity", (65, 449, 1000))])
def test_row_reduction_and_camera_position_chain(pose, counts):
    from gsplatloc_amd.synthetic import replica_intrinsics
    c2w = _f32(POSES[pose]) if pose != "identity" else torch.eye(4, dtype=torch.float64)
    V64 = _f32(torch.linalg.inv(c2w))
    V, K = V64.float().contiguous().to(DEV), replica_intrinsics(160, 120).contiguous().to(DEV)
    g = torch.Generator().manual_seed(5)
    rule = Rule(f"pose row reduction {pose}")
    for n in counts:
        rows = _rows(n, seed=1000 + n)
        part = torch.rand(37, 2, generator=g) + 0.1
        nsum = torch.rand(1, generator=g) * 100
        out = _pack(rows.to(DEV), n, V, K, part.to(DEV), 37, nsum.to(DEV)).cpu()
        assert bool(torch.isfinite(out).all()), (n, out)
        tot64 = rows[:n, :15].double().sum(0)
        tot32 = rows[:n, :15].sum(0)
        want, floor = _chain(tot64, V64), _chain(tot32, V64)
        rule.add("v_viewmat", out[:12], want, floor, case=f"n {n}")
        rule.add("loss sums", out[12:14], part.double().sum(0), part.sum(0), case=f"n {n}")
        assert float(out[14]) == float(nsum) and float(out[15]) == 0.0
        if pose == "identity":  # R = I, t = 0: the chain vanishes, what is left is the sum
            plain = torch.cat([tot64[:9].reshape(3, 3), (tot64[9:12] - tot64[12:15])[:, None]], 1).reshape(12)
            rule.add("v_viewmat (no chain)", out[:12], plain, torch.cat(
                [tot32[:9].reshape(3, 3), (tot32[9:12] - tot32[12:15])[:, None]], 1).reshape(12), case=f"n {n}")
    rule.finish()


# ------------------------------------------------------------------------------------------- g. two routes, one result
def test_rows_route_and_packed_route_are_bit_identical():
    """One rank: gsl_pose_step sums vm_rows and loss_partials itself.  Several ranks: gsl_pack_pose_reduce sums them and
    the step takes the reduced 16 floats.  Same fixed order of every sum, so the same bits."""
    from gsplatloc_amd.synthetic import replica_intrinsics
    init = _f32(POSES["m00"])
    W, H, n, nb = 160, 120, 449, 70
    hp = PoseHyper(width=W, height=H, depth_w=0.7, edge_w=0.25, normal_w=0.05, max_steps=25)
    K = replica_intrinsics(W, H).contiguous().to(DEV)
    a = Device(hp, init @ small_pose(0.3, 0.01)).init(init)
    b = Device(hp, init @ small_pose(0.3, 0.01)).init(init)
    g = torch.Generator().manual_seed(9)
    for k in range(5):
        rows = (_rows(n, seed=50 + k) * 10.0).to(DEV)
        part = (torch.rand(nb, 2, generator=g) * 300 + 1).to(DEV)
        nsum = (torch.rand(1, generator=g) * 3 * H).to(DEV)
        a.step(rows=rows, n_rows=n, K=K, partials=part, n_partials=nb, normal_sum=nsum)
        out16 = _pack(rows, n, b.viewmat, K, part, nb, nsum)
        b.step(v_viewmat=out16, loss_sums=out16[12:])
        sa, sb = a.state(), b.state()
        assert not _same_bits(sa, sb), (k, _same_bits(sa, sb))
        assert int(sa["i"][0]) == k + 1 and math.isfinite(float(sa["f"][28]))
    assert float((sa["f"][4:7].double() - init[:3, 3]).norm()) > 1e-3  # and the pose moved
