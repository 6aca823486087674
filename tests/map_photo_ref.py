"""numpy mirror of csrc/map_photo.hip: the intensity image of gsl_map_photo_intensity, the 30 integers and the two extra
words of gsl_map_pose_info_photo -- the point-to-plane equation of csrc/map_info.hip and the photometric equation of a
used row, summed into the same fixed-point slots -- and the two alignments on those sums, in float32 with every
operation rounded once in the device's order (numpy's float32 multiply, add, subtract, divide, sqrt and rint are the
IEEE operations, and nothing here is fused).  Its own copy of the row rule, geometry included, as the other mirrors
have; the float64 Gauss-Newton step is tests/map_align_ref.step, imported unchanged.

And the scene the feature is for: a textured wall, where depth alone leaves three moves of the camera open."""
import numpy as np

from tests import map_align_ref as align
from tests.map_align_batch_ref import done_of
from tests.map_free_ref import keep_of, w2c_of  # noqa: F401
from tests.map_score_ref import beyond_of  # noqa: F401

F32, F64 = np.float32, np.float64
VALUES = 30
ONE = F32(1048576.0)  # 2^20
MAX_DEPTH = F32(64.0)
PHOTO_MAX_A = F32(8.0)
PHOTO_MAX_DEPTH = F32(16.0)
PHOTO_MAX_SCALE = 16.0
SLOTS = [(a, b) for a in range(6) for b in range(a, 6)] + [(a, 6) for a in range(6)] + [(6, 6)]  # J_6 = r
WR, WG, WB = F32(0.299), F32(0.587), F32(0.114)


def intensity(rgb):
    """gsl_map_photo_intensity: rgb [H,W,3] in 0 .. 255 -> float32 [H,W]."""
    c = np.asarray(rgb, dtype=F32)
    with np.errstate(all="ignore"):
        y = ((WR * c[..., 0] + WG * c[..., 1]) + WB * c[..., 2]) / F32(255.0)
    assert y.dtype == F32
    return y


def in01(t):
    return (t >= F32(0)) & (t <= F32(1))


def rows(means, colors, w2c, intr, depth, image, keep, beyond, kappa, near, scale, max_residual):
    """(tested [n], used [n], J [n,7] float32, photo [n], Jc [n,7] float32; garbage where the flag is false).  The rule:
    the headers of csrc/map_info.hip and csrc/map_photo.hip."""
    p = np.asarray(means, dtype=F32).reshape(-1, 3)
    col = np.asarray(colors, dtype=F32).reshape(-1, 3)
    w = np.asarray(w2c, dtype=F32).reshape(4, 4)
    depth, Y = np.asarray(depth, dtype=F32), np.asarray(image, dtype=F32)
    H, W = depth.shape
    assert Y.shape == depth.shape and len(col) == len(p)
    fx, fy, cx, cy = (F32(a) for a in intr)
    keep, beyond, kappa, near = F32(keep), F32(beyond), F32(kappa), F32(near)
    s, rmax = F32(scale), F32(max_residual)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    one, half = F32(1), F32(0.5)
    zeros = np.zeros((len(p), 7), F32)
    with np.errstate(all="ignore"):
        x, y, z = (((w[j, 0] * px + w[j, 1] * py) + w[j, 2] * pz) + w[j, 3] for j in range(3))
        u, v = fx * x / z + cx, fy * y / z + cy
        uf, vf = np.rint(u), np.rint(v)  # round half to even
        inner = (z > near) & (uf >= one) & (uf <= F32(W - 2)) & (vf >= one) & (vf <= F32(H - 2))
        if not inner.any():
            return inner, inner.copy(), zeros, inner.copy(), zeros.copy()
        ufi, vfi = np.where(inner, uf, one), np.where(inner, vf, one)
        uc, vc = ufi.astype(np.int64), vfi.astype(np.int64)
        d0 = depth[vc, uc]
        tested = inner & (d0 > F32(0)) & (d0 < F32(np.inf))
        lo, hi = d0 * keep, d0 * beyond
        used = tested & (z >= lo) & (z <= hi) & (z < MAX_DEPTH)
        dl, dr, du, dd = depth[vc, uc - 1], depth[vc, uc + 1], depth[vc - 1, uc], depth[vc + 1, uc]
        for d in (dl, dr, du, dd):
            used &= (d > F32(0)) & (d < F32(np.inf)) & (d >= lo) & (d <= hi)
        i0 = one / d0
        s0, tol = i0 + i0, kappa * i0
        su, sv = one / dl + one / dr, one / du + one / dd
        used &= (np.abs(su - s0) <= tol) & (np.abs(sv - s0) <= tol)
        kx0, ky0 = (ufi - cx) / fx, (vfi - cy) / fy
        kxl, kxr = ((ufi - one) - cx) / fx, ((ufi + one) - cx) / fx
        kyu, kyd = ((vfi - one) - cy) / fy, ((vfi + one) - cy) / fy
        ax, ay, az = kxr * dr - kxl * dl, ky0 * dr - ky0 * dl, dr - dl
        bx, by, bz = kx0 * dd - kx0 * du, kyd * dd - kyu * du, dd - du
        c0, c1, c2 = ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx
        length = np.sqrt((c0 * c0 + c1 * c1) + c2 * c2)
        used &= length > F32(0)
        n0, n1, n2 = c0 / length, c1 / length, c2 / length
        e0, e1, e2 = x - kx0 * d0, y - ky0 * d0, z - d0
        J = np.stack([y * n2 - z * n1, z * n0 - x * n2, x * n1 - y * n0, n0, n1, n2,
                      (n0 * e0 + n1 * e1) + n2 * e2], axis=1)
        # the photometric equation, where the geometric one exists
        Yi = (WR * col[:, 0] + WG * col[:, 1]) + WB * col[:, 2]
        Y0, Yl, Yr, Yu, Yd = Y[vc, uc], Y[vc, uc - 1], Y[vc, uc + 1], Y[vc - 1, uc], Y[vc + 1, uc]
        photo = used & in01(Yi) & in01(Y0) & in01(Yl) & in01(Yr) & in01(Yu) & in01(Yd)
        gx, gy = (Yr - Yl) * half, (Yd - Yu) * half
        Yp = (Y0 + gx * (u - ufi)) + gy * (v - vfi)
        rc = Yp - Yi
        photo &= np.abs(rc) <= rmax
        a0, a1 = (s * gx) * fx / z, (s * gy) * fy / z
        a2 = -((a0 * x + a1 * y) / z)
        photo &= (np.abs(a0) <= PHOTO_MAX_A) & (np.abs(a1) <= PHOTO_MAX_A) & (np.abs(a2) <= PHOTO_MAX_A)
        photo &= z < PHOTO_MAX_DEPTH
        Jc = np.stack([y * a2 - z * a1, z * a0 - x * a2, x * a1 - y * a0, a0, a1, a2, s * rc], axis=1)
        assert J.dtype == F32 and Jc.dtype == F32 and Yi.dtype == F32
    return tested, used, J, photo, Jc


def fixed(Ja, a, b):
    scaled = (Ja[:, a] * Ja[:, b]) * ONE  # one float32 product, then an exact scaling
    assert scaled.dtype == F32
    return int(np.rint(scaled).astype(np.int64).sum())  # round half to even


def pose_info(means, colors, w2c, intr, depth, image, keep, beyond, kappa, near, scale, max_residual):
    """What gsl_map_pose_info_photo leaves: (out int64 [30], extra int64 [2])."""
    tested, used, J, photo, Jc = rows(means, colors, w2c, intr, depth, image, keep, beyond, kappa, near, scale,
                                      max_residual)
    out, extra = np.zeros(VALUES, dtype=np.int64), np.zeros(2, dtype=np.int64)
    Ju, Jp = J[used], Jc[photo]
    with np.errstate(all="ignore"):
        for slot, (a, b) in enumerate(SLOTS):
            out[slot] = fixed(Ju, a, b) + fixed(Jp, a, b)
        extra[0], extra[1] = photo.sum(), fixed(Jp, 6, 6)
    out[28], out[29] = used.sum(), tested.sum()
    return out, extra


def max_rows(intr, width, height, keep, scale, max_residual):
    """gsl_map_info_photo_max_rows in float64, as the entry point computes it."""
    fx, fy, cx, cy = (float(F32(a)) for a in intr)
    tx = max(abs(0.5 - cx), abs(width - 1.5 - cx)) / abs(fx)
    ty = max(abs(0.5 - cy), abs(height - 1.5 - cy)) / abs(fy)
    S = np.sqrt(1.0 + tx * tx + ty * ty)
    B = 1.01 * 64.0 * S * (1.0 + 1.0 / float(F32(keep)))
    Bc = 1.01 * max(16.0 * S * 8.0 * np.sqrt(3.0), float(F32(scale)) * float(F32(max_residual)))
    rows_ = 9223372036854775807.0 / ((B * B + Bc * Bc) * 1048576.0 + 2.0)
    return int(rows_) if rows_ < 2147483647.0 else 0x7FFFFFFF


def unpack(out):
    """(H [6,6], g [6], rss, used, tested) in float64 from the 30 integers."""
    out = np.asarray(out, dtype=np.int64)
    H = np.zeros((6, 6))
    for slot, (a, b) in enumerate(SLOTS[:21]):
        H[a, b] = H[b, a] = float(out[slot]) / 1048576.0
    return H, out[21:27].astype(np.float64) / 1048576.0, float(out[27]) / 1048576.0, int(out[28]), int(out[29])


def pose_align(means, colors, w2c, intr, depth, image, keep, beyond, kappa, near, scale, max_residual, max_steps,
               damping, min_used, max_rot, max_trans, eps_rot, eps_trans):
    """What gsl_map_pose_align_photo leaves: tests/map_align_ref.pose_align's tuple, on these sums."""
    assert 1 <= max_steps <= align.MAX_STEPS and min_used >= 7
    w = np.asarray(w2c, dtype=F32).reshape(4, 4)
    work = np.zeros((4, 4), F32)
    work[:3], work[3, 3] = w[:3], 1.0
    P = work[:3].astype(F64)
    flags = [0, 0]
    hist, xis = np.zeros((max_steps, 4), np.int64), np.zeros((max_steps, 6), F64)
    sums, at = None, -1
    for k in range(max_steps):
        if at != flags[0]:  # a pose that has not moved gives the same 30 integers again
            sums, at = pose_info(means, colors, work, intr, depth, image, keep, beyond, kappa, near, scale,
                                 max_residual)[0], flags[0]
        align.step(sums, k, P, work, flags, hist, xis, damping, min_used, max_rot, max_trans, eps_rot, eps_trans)
    return P, work, flags[0], flags[1], hist, xis, sums


def pose_align_batch(means, colors, w2cs, *args):
    """Per pose of w2cs [k,4,4] what gsl_map_pose_align_batch_photo leaves (tests/map_align_batch_ref.py: the done word
    and the sums follow from the single call's history)."""
    out = []
    for w2c in np.asarray(w2cs, dtype=F32).reshape(-1, 4, 4):
        P, work, taken, _, hist, xis, sums = pose_align(means, colors, w2c, *args)
        out.append((P, work, taken, done_of(hist), hist, xis, np.asarray(sums, dtype=np.int64)))
    return out


# ---- the textured wall --------------------------------------------------------------------------------------------
WALL_W, WALL_H = 160, 120
WALL_INTR = (80.0, 80.0, 79.5, 59.5)


def texture(P):
    """Intensity in 0.1 .. 0.9 of the world point P [..., 3] (float64): smooth, with a gradient in both directions of
    the wall."""
    X, Y, Z = P[..., 0], P[..., 1], P[..., 2]
    return 0.5 + 0.15 * np.sin(3.1 * X + 0.7 * Y) + 0.15 * np.cos(4.3 * Y - 1.3 * X) + 0.1 * np.sin(3.95 * X + 3.57 * Y + Z)


def wall_frame(c2w, slant=0.0, width=WALL_W, height=WALL_H, intr=WALL_INTR):
    """(depth float32 [H,W], rgb float32 [H,W,3] in 0 .. 255) of the wall z = 2 + slant * x seen from c2w [4,4]
    (float64): the rays are cast in float64, the depth is rounded to float32, the colour is grey, the texture of the
    world point."""
    fx, fy, cx, cy = intr
    v, u = np.mgrid[0:height, 0:width].astype(F64)
    dirs = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)
    c2w = np.asarray(c2w, dtype=F64)
    R, t = c2w[:3, :3], c2w[:3, 3]
    dw = dirs @ R.T
    n = np.array([-slant, 0.0, 1.0])
    lam = (2.0 - n @ t) / (dw @ n)  # the camera's z: dirs has z = 1
    grey = texture(t + lam[..., None] * dw) * 255.0
    return lam.astype(F32), np.repeat(grey[..., None], 3, axis=-1).astype(F32)


def wall_map(depth, rgb, intr=WALL_INTR):
    """(means float32 [n,3], colors float32 [n,3]) of a frame at the identity: k_map_append's back-projection and its
    rgb / 255."""
    d = np.asarray(depth, F32)
    v, u = np.mgrid[0:d.shape[0], 0:d.shape[1]]
    fx, fy, cx, cy = (F32(a) for a in intr)
    means = np.stack([(u.astype(F32) - cx) / fx * d, (v.astype(F32) - cy) / fy * d, d], -1).reshape(-1, 3)
    return means, (np.asarray(rgb, F32) / F32(255.0)).reshape(-1, 3)


def twist_pose(xi):
    """float64 [4,4] exp(xi^), xi = (omega [rad], upsilon [m])."""
    w, t = np.asarray(xi[:3], F64), np.asarray(xi[3:], F64)
    th = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    T = np.eye(4)
    if th < 1e-12:
        T[:3, :3], T[:3, 3] = np.eye(3) + K, t
        return T
    T[:3, :3] = np.eye(3) + np.sin(th) / th * K + (1.0 - np.cos(th)) / th ** 2 * (K @ K)
    T[:3, 3] = (np.eye(3) + (1.0 - np.cos(th)) / th ** 2 * K + (th - np.sin(th)) / th ** 3 * (K @ K)) @ t
    return T


WALL_MOVE = np.array([0.0, 0.0, np.deg2rad(0.3), 0.012, -0.008, 0.0])  # the second frame's camera-to-world pose


def wall_case(slant=0.0, width=WALL_W, height=WALL_H, intr=WALL_INTR, move=WALL_MOVE):
    """The map is frame 0 (the identity) back-projected; the query is the frame at exp(move^): 0.3 degrees about the
    optical axis and 14.4 mm in the plane.  dict(means, colors, depth, image, truth [4,4] float64 camera to world)."""
    d0, rgb0 = wall_frame(np.eye(4), slant, width, height, intr)
    truth = twist_pose(move)
    d1, rgb1 = wall_frame(truth, slant, width, height, intr)
    means, colors = wall_map(d0, rgb0, intr)
    return dict(means=means, colors=colors, depth=d1, rgb=rgb1, image=intensity(rgb1), truth=truth, intr=intr)


def pose_error(w2c, truth):
    """(metres, degrees) between the world-to-camera pose w2c [3 or 4,4] and the camera-to-world truth."""
    M = np.eye(4)
    M[:3] = np.asarray(w2c, F64)[:3]
    c2w = np.linalg.inv(M)
    R = c2w[:3, :3].T @ truth[:3, :3]
    ang = np.degrees(np.arccos(min(1.0, max(-1.0, (np.trace(R) - 1.0) / 2.0))))
    return float(np.linalg.norm(c2w[:3, 3] - truth[:3, 3])), float(ang)
