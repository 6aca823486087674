"""numpy mirror of csrc/map_info.hip: the 30 integers of gsl_map_pose_info -- the fixed-point upper triangle of
H = sum J J^T, g = sum J r, sum r^2, rows used, rows tested -- in float32 with every operation rounded once in the
device's order (numpy's float32 multiply, add, subtract, divide, sqrt and rint are the IEEE operations, and nothing
here is fused), with its own copy of the row rule as the other mirrors have; and what the host makes of them."""
import numpy as np

from tests.map_free_ref import keep_of, w2c_of  # noqa: F401  (keep = 1 - rho; the float64 inverse rounded to float32)
from tests.map_score_ref import beyond_of  # noqa: F401  (beyond = 1 + rho)

F32 = np.float32
VALUES = 30
ONE = F32(1048576.0)  # 2^20
MAX_DEPTH = F32(64.0)
SLOTS = [(a, b) for a in range(6) for b in range(a, 6)] + [(a, 6) for a in range(6)] + [(6, 6)]  # J_6 = r
assert len(SLOTS) == 28


def rows(means, w2c, intr, depth, keep, beyond, kappa, near):
    """(tested [n] bool, used [n] bool, J [n,7] float32 = (m, n, r); garbage where not used).  The rule: the header of
    csrc/map_info.hip."""
    p = np.asarray(means, dtype=F32).reshape(-1, 3)
    w = np.asarray(w2c, dtype=F32).reshape(4, 4)
    depth = np.asarray(depth, dtype=F32)
    H, W = depth.shape
    fx, fy, cx, cy = (F32(a) for a in intr)
    keep, beyond, kappa, near = F32(keep), F32(beyond), F32(kappa), F32(near)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    one = F32(1)
    with np.errstate(all="ignore"):
        x, y, z = (((w[j, 0] * px + w[j, 1] * py) + w[j, 2] * pz) + w[j, 3] for j in range(3))
        u, v = fx * x / z + cx, fy * y / z + cy
        uf, vf = np.rint(u), np.rint(v)  # round half to even
        assert uf.dtype == F32 and vf.dtype == F32 and z.dtype == F32
        inner = (z > near) & (uf >= one) & (uf <= F32(W - 2)) & (vf >= one) & (vf <= F32(H - 2))
        if not inner.any():  # (also an image without an inner pixel: nothing to index)
            return inner, inner.copy(), np.zeros((len(p), 7), F32)
        uf, vf = np.where(inner, uf, one), np.where(inner, vf, one)
        uc, vc = uf.astype(np.int64), vf.astype(np.int64)
        d0 = depth[vc, uc]
        tested = inner & (d0 > F32(0)) & (d0 < F32(np.inf))
        lo, hi = d0 * keep, d0 * beyond  # one rounded product each
        used = tested & (z >= lo) & (z <= hi) & (z < MAX_DEPTH)
        dl, dr, du, dd = depth[vc, uc - 1], depth[vc, uc + 1], depth[vc - 1, uc], depth[vc + 1, uc]
        for d in (dl, dr, du, dd):
            used &= (d > F32(0)) & (d < F32(np.inf)) & (d >= lo) & (d <= hi)
        i0 = one / d0
        s0, tol = i0 + i0, kappa * i0
        su, sv = one / dl + one / dr, one / du + one / dd
        used &= (np.abs(su - s0) <= tol) & (np.abs(sv - s0) <= tol)
        kx0, ky0 = (uf - cx) / fx, (vf - cy) / fy
        kxl, kxr = ((uf - one) - cx) / fx, ((uf + one) - cx) / fx
        kyu, kyd = ((vf - one) - cy) / fy, ((vf + one) - cy) / fy
        ax, ay, az = kxr * dr - kxl * dl, ky0 * dr - ky0 * dl, dr - dl
        bx, by, bz = kx0 * dd - kx0 * du, kyd * dd - kyu * du, dd - du
        c0, c1, c2 = ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx
        length = np.sqrt((c0 * c0 + c1 * c1) + c2 * c2)
        used &= length > F32(0)
        n0, n1, n2 = c0 / length, c1 / length, c2 / length
        e0, e1, e2 = x - kx0 * d0, y - ky0 * d0, z - d0
        J = np.stack([y * n2 - z * n1, z * n0 - x * n2, x * n1 - y * n0, n0, n1, n2,
                      (n0 * e0 + n1 * e1) + n2 * e2], axis=1)
        assert J.dtype == F32 and length.dtype == F32
    return tested, used, J


def pose_info(means, w2c, intr, depth, keep, beyond, kappa, near):
    """What gsl_map_pose_info leaves in out: int64 [30]."""
    tested, used, J = rows(means, w2c, intr, depth, keep, beyond, kappa, near)
    out = np.zeros(VALUES, dtype=np.int64)
    Ju = J[used]
    for slot, (a, b) in enumerate(SLOTS):
        scaled = (Ju[:, a] * Ju[:, b]) * ONE  # one float32 product, then an exact scaling
        assert scaled.dtype == F32
        out[slot] = np.rint(scaled).astype(np.int64).sum()  # round half to even; |scaled| < 2^53: the conversion is exact
    out[28], out[29] = used.sum(), tested.sum()
    return out


def max_rows(intr, width, height, keep):
    """gsl_map_info_max_rows in float64, as the entry point computes it."""
    fx, fy, cx, cy = (float(F32(a)) for a in intr)
    tx = max(abs(0.5 - cx), abs(width - 1.5 - cx)) / abs(fx)
    ty = max(abs(0.5 - cy), abs(height - 1.5 - cy)) / abs(fy)
    B = 1.01 * 64.0 * np.sqrt(1.0 + tx * tx + ty * ty) * (1.0 + 1.0 / float(F32(keep)))
    rows_ = 9223372036854775807.0 / (B * B * 1048576.0 + 1.0)
    return int(rows_) if rows_ < 2147483647.0 else 0x7FFFFFFF


def unpack(out):
    """(H [6,6], g [6], rss, used, tested) in float64 from the 30 integers."""
    out = np.asarray(out, dtype=np.int64)
    H = np.zeros((6, 6))
    for slot, (a, b) in enumerate(SLOTS[:21]):
        H[a, b] = H[b, a] = float(out[slot]) / 1048576.0
    return H, out[21:27].astype(np.float64) / 1048576.0, float(out[27]) / 1048576.0, int(out[28]), int(out[29])
