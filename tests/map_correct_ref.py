"""The numpy mirror of csrc/map_correct.hip (the rule: include/gsloc_hip.h, "trajectory correction") -- float32, one
rounding per operation, in the kernel's order, with its skip conditions -- and a float64 reference of
``mapping.spread_correction`` that shares nothing with it: the logarithm and the exponential are those of a generic 4x4
matrix (scipy's where it is installed, else a scaling-and-squaring Taylor series and a Newton iteration on it), not the
closed forms of SE(3)."""
import numpy as np

F32 = np.float32
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F32)


def table_of(transforms):
    """[n,4,4] -> the float32 [n,12] table ``GaussianMap.correct`` uploads: the upper 3 x 4 of each, rounded once."""
    return np.ascontiguousarray(np.asarray(transforms, np.float64)[:, :3, :].astype(F32).reshape(-1, 12))


def correct(means, origins, table):
    """means [n,3] float32, origins [n] int32, table [n_frames,12] float32 -> dict(means: the corrected copy, moved /
    outside: bool [n], counters: (rows moved, rows outside the table))."""
    p = np.array(means, F32).reshape(-1, 3)
    o = np.asarray(origins, np.int64).reshape(-1)
    t = np.asarray(table, F32).reshape(-1, 12)
    assert len(o) == len(p) and t.dtype == F32 and p.dtype == F32
    outside = (o < 0) | (o >= len(t))
    e = t[np.where(outside, 0, o)]  # [n,12]; the rows outside are masked below
    with np.errstate(invalid="ignore"):
        finite = (np.abs(p) < F32(np.inf)).all(axis=1)
        identity = (e == IDENTITY[None]).all(axis=1)  # twelve ==: -0.0 is 0, a NaN is not
    moved = ~outside & finite & ~identity
    out = p.copy()
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        for a in range(3):
            r = e[:, 4 * a:4 * a + 4]
            new = ((r[:, 0] * x + r[:, 1] * y) + r[:, 2] * z) + r[:, 3]  # float32 arrays: each operation rounds once
            assert new.dtype == F32
            out[moved, a] = new[moved]
    return dict(means=out, moved=moved, outside=outside, counters=(int(moved.sum()), int(outside.sum())))


# ---- the float64 reference of spread_correction ---------------------------------------------------------------------
def _expm(A):
    try:
        from scipy.linalg import expm
        return np.asarray(expm(A), np.float64)
    except ImportError:
        k = max(0, int(np.ceil(np.log2(max(np.abs(A).sum(axis=1).max(), 1e-300)))) + 4)
        B, term, out = A / 2.0 ** k, np.eye(len(A)), np.eye(len(A))
        for j in range(1, 30):
            term = term @ B / j
            out = out + term
        for _ in range(k):
            out = out @ out
        return out


def _logm(A):
    try:
        from scipy.linalg import logm
        return np.real(np.asarray(logm(A))).astype(np.float64)
    except ImportError:
        X = A - np.eye(len(A))
        for _ in range(60):  # Newton on exp(X) = A: quadratic, since every iterate is a function of A
            X = X - np.eye(len(A)) + _expm(-X) @ A
        return X


def spread(poses, first, last, delta, by="path"):
    """[n,4,4] float64: D_k = expm(s_k logm(delta)), s_k the share of the camera centres' path from first to last that
    lies before k (0 up to first, 1 from last on; the share of the frames when the path has no length or by="index")."""
    P, D = np.asarray(poses, np.float64), np.asarray(delta, np.float64)
    n = len(P)
    L = _logm(D)
    s = np.zeros(n)
    for k in range(n):
        if k >= last:
            s[k] = 1.0
        elif k > first:
            s[k] = (k - first) / (last - first)
    if by == "path":
        c = P[:, :3, 3]
        length = lambda a, b: sum(float(np.linalg.norm(c[j + 1] - c[j])) for j in range(a, b))  # noqa: E731
        total = length(first, last)
        if total > 0.0:
            for k in range(first + 1, last):
                s[k] = length(first, k) / total
    return np.stack([_expm(s[k] * L) for k in range(n)]), s


# ---- drifting trajectories, shared by the CPU and the GPU tests -----------------------------------------------------
def twist(rot_deg, trans, axis=(0.3, 1.0, -0.2), direction=(0.6, 0.1, 0.8)):
    """float64 [4,4]: a turn by rot_deg about ``axis`` and a shift by ``trans`` metres along ``direction``."""
    ax = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    th = np.radians(rot_deg)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    step = np.eye(4)
    step[:3, :3] = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)
    step[:3, 3] = trans * np.asarray(direction, np.float64) / np.linalg.norm(direction)
    return step


def circle_poses(n, radius=0.5):
    """float64 [n,4,4]: n cameras evenly on a circle of that radius in the x-z plane, each looking outwards."""
    out = np.tile(np.eye(4), (n, 1, 1))
    for k in range(n):
        a = 2.0 * np.pi * k / n
        c, s = np.cos(a), np.sin(a)
        out[k, :3, :3] = [[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]
        out[k, :3, 3] = [radius * s, 0.0, radius * c]
    return out


def drifted(true, rot_deg, trans):
    """float64 [n,4,4]: the trajectory of a tracker that starts at true[0] and adds the same body-frame error -- rot_deg
    and ``trans`` metres -- to every frame-to-frame motion."""
    err, out = twist(rot_deg, trans), [np.asarray(true[0], np.float64)]
    for k in range(len(true) - 1):
        out.append(out[-1] @ np.linalg.inv(true[k]) @ true[k + 1] @ err)
    return np.stack(out)


def room_loop(n=8, rot_deg=0.3, trans=0.005, centre=(0.6, 0.1, 0.8), radius=0.1, yaw_deg=35.0, sway_deg=3.0):
    """(true poses, drifted poses), float64 [n,4,4]: a short loop in the box room of gsplatloc_amd.synthetic -- the camera
    on a circle of that radius about ``centre`` in the x-z plane, looking at a corner (yaw about y) and swaying by
    sway_deg; frame n - 1 stands one step short of frame 0 and sees what frame 0 saw."""
    true = np.tile(np.eye(4), (n, 1, 1))
    for k in range(n):
        a = 2.0 * np.pi * k / n
        yaw = np.radians(yaw_deg + sway_deg * np.sin(a))
        c, s = np.cos(yaw), np.sin(yaw)
        true[k, :3, :3] = [[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]
        true[k, :3, 3] = [centre[0] + radius * (np.cos(a) - 1.0), centre[1], centre[2] + radius * np.sin(a)]
    return true, drifted(true, rot_deg, trans)


def rms(x):
    return float(np.sqrt(np.mean(np.sum(np.square(np.asarray(x, np.float64)), axis=-1))))
