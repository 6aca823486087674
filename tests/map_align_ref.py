"""numpy mirror of csrc/map_align.hip: per iteration the 30 integers of tests/map_info_ref.py at the float32 working pose,
then k_map_align_step in float64 -- numpy's float64 add, subtract, multiply and divide are the IEEE operations and
nothing here is fused -- with every operation in the order the kernel's header writes down.  There is no sine, cosine
or square root in it (the retraction is the Cayley map), so the pose, the working copy and the history are the device's
bit for bit."""
import numpy as np

from tests import map_info_ref as info

F32, F64 = np.float32, np.float64
MAX_STEPS = 32
STEPPED, CONVERGED, FEW, SINGULAR, TOO_FAR = range(5)
NAMES = ("STEPPED", "CONVERGED", "FEW", "SINGULAR", "TOO_FAR")
ONE = F64(1048576.0)


def solve(sums, damping):
    """xi [6] float64 of (H + damping * used * I) xi = -g by the kernel's LDL^T; None when a pivot is not above 0."""
    sums = np.asarray(sums, dtype=np.int64)
    A = np.zeros((6, 6), F64)
    slot = 0
    for a in range(6):
        for c in range(a, 6):
            A[a, c] = A[c, a] = F64(int(sums[slot])) / ONE
            slot += 1
    lam = F64(damping) * F64(int(sums[28]))
    b = np.zeros(6, F64)
    for a in range(6):
        A[a, a] = A[a, a] + lam
        b[a] = -(F64(int(sums[21 + a])) / ONE)
    L, D = np.zeros((6, 6), F64), np.zeros(6, F64)
    for j in range(6):
        d = A[j, j]
        for q in range(j):
            d = d - (L[j, q] * L[j, q]) * D[q]
        if not d > 0.0:
            return None
        D[j] = d
        for i in range(j + 1, 6):
            s = A[i, j]
            for q in range(j):
                s = s - (L[i, q] * L[j, q]) * D[q]
            L[i, j] = s / d
    z, x = np.zeros(6, F64), np.zeros(6, F64)
    for i in range(6):
        v = b[i]
        for q in range(i):
            v = v - L[i, q] * z[q]
        z[i] = v
    for i in range(5, -1, -1):
        v = z[i] / D[i]
        for q in range(i + 1, 6):
            v = v - L[q, i] * x[q]
        x[i] = v
    return x


def cayley(omega):
    """R [3,3] float64 of the kernel's retraction."""
    a0, a1, a2 = (F64(w) * F64(0.5) for w in omega)
    s = (a0 * a0 + a1 * a1) + a2 * a2
    c, den = F64(1.0) - s, F64(1.0) + s
    two = F64(2.0)
    t00, t11, t22 = (a0 * a0) * two, (a1 * a1) * two, (a2 * a2) * two
    t01, t02, t12 = (a0 * a1) * two, (a0 * a2) * two, (a1 * a2) * two
    u0, u1, u2 = a0 * two, a1 * two, a2 * two
    return np.array([[(c + t00) / den, (t01 - u2) / den, (t02 + u1) / den],
                     [(t01 + u2) / den, (c + t11) / den, (t12 - u0) / den],
                     [(t02 - u1) / den, (t12 + u0) / den, (c + t22) / den]], dtype=F64)


def retract(P, xi):
    """[R | upsilon] P for P [3,4] float64."""
    R, Q = cayley(xi[:3]), np.zeros((3, 4), F64)
    for i in range(3):
        for j in range(4):
            Q[i, j] = (R[i, 0] * P[0, j] + R[i, 1] * P[1, j]) + R[i, 2] * P[2, j]
        Q[i, 3] = Q[i, 3] + xi[3 + i]
    return Q


def dot3(v):
    return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]


def step(sums, k, P, work, flags, rows, xis, damping, min_used, max_rot, max_trans, eps_rot, eps_trans):
    """k_map_align_step on the mirror's state: P [3,4] float64, work [4,4] float32, flags [steps_taken, done], rows
    [max_steps,4] int64 and xis [max_steps,6] float64, all changed in place."""
    sums = np.asarray(sums, dtype=np.int64)
    rows[k, 1:], xis[k] = (sums[28], sums[29], sums[27]), 0.0
    if flags[1]:
        rows[k, 0] = rows[k - 1, 0]
        return
    if sums[28] < min_used:
        rows[k, 0], flags[1] = FEW, 1
        return
    with np.errstate(all="ignore"):
        x = solve(sums, damping)
        if x is None:
            rows[k, 0], flags[1] = SINGULAR, 1
            return
        ww, vv = dot3(x[:3]), dot3(x[3:])
        xis[k] = x
        if not (ww <= F64(max_rot) * F64(max_rot) and vv <= F64(max_trans) * F64(max_trans)):
            rows[k, 0], flags[1] = TOO_FAR, 1
            return
        P[:] = retract(P, x)
        work[:3] = P.astype(F32)  # round to nearest even
        flags[0] += 1
        converged = bool(ww <= F64(eps_rot) * F64(eps_rot) and vv <= F64(eps_trans) * F64(eps_trans))
    rows[k, 0] = CONVERGED if converged else STEPPED
    if converged:
        flags[1] = 1


def pose_align(means, w2c, intr, depth, keep, beyond, kappa, near, max_steps, damping, min_used, max_rot, max_trans,
               eps_rot, eps_trans):
    """What gsl_map_pose_align leaves: (P [3,4] float64, work [4,4] float32, steps_taken, done, rows [max_steps,4] int64
    = (status, used, tested, rss_fixed), xis [max_steps,6] float64, sums [30] int64 of the last iteration)."""
    assert 1 <= max_steps <= MAX_STEPS and min_used >= 7
    w = np.asarray(w2c, dtype=F32).reshape(4, 4)
    work = np.zeros((4, 4), F32)
    work[:3], work[3, 3] = w[:3], 1.0
    P = work[:3].astype(F64)
    flags = [0, 0]
    rows, xis = np.zeros((max_steps, 4), np.int64), np.zeros((max_steps, 6), F64)
    sums, at = None, -1
    for k in range(max_steps):
        if at != flags[0]:  # a pose that has not moved gives the same 30 integers again
            sums, at = info.pose_info(means, work, intr, depth, keep, beyond, kappa, near), flags[0]
        step(sums, k, P, work, flags, rows, xis, damping, min_used, max_rot, max_trans, eps_rot, eps_trans)
    return P, work, flags[0], flags[1], rows, xis, sums
