"""numpy mirror of csrc/map_score.hip: per pose the live rows a depth frame tests, those that agree with it and those
in front of it, in float32 with every operation rounded once in the device's order (numpy's float32 multiply, add,
divide and rint are the IEEE operations, and nothing here is fused).  The projection up to (uf, vf) is that of
tests/map_free_ref.py."""
import numpy as np

from tests.map_free_ref import keep_of, w2c_of  # noqa: F401  (keep = 1 - rho; the float64 inverse rounded to float32)

F32 = np.float32


def beyond_of(rho):
    """beyond = 1 + rho, the float32 value the host computes."""
    return F32(1.0) + F32(rho)


def verdicts(means, w2c, intr, depth, keep, beyond, near):
    """One pose: (tested, agree, front, behind), bool [n] each.  x = ((w0 px + w1 py) + w2 pz) + w3 (y, z likewise);
    u = fx x / z + cx, v = fy y / z + cy; uf = rint(u), vf = rint(v); tested = z > near and 0 <= uf <= W - 1 and
    0 <= vf <= H - 1 and d = depth[vf, uf] is finite and > 0; front = tested and z < d * keep; behind = tested and
    z > d * beyond; agree = tested and neither."""
    p = np.asarray(means, dtype=F32).reshape(-1, 3)
    w = np.asarray(w2c, dtype=F32).reshape(4, 4)
    depth = np.asarray(depth, dtype=F32)
    H, W = depth.shape
    fx, fy, cx, cy = (F32(a) for a in intr)
    keep, beyond, near = F32(keep), F32(beyond), F32(near)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        x, y, z = (((w[j, 0] * px + w[j, 1] * py) + w[j, 2] * pz) + w[j, 3] for j in range(3))
        u, v = fx * x / z + cx, fy * y / z + cy
        uf, vf = np.rint(u), np.rint(v)  # round half to even
        assert uf.dtype == F32 and vf.dtype == F32 and z.dtype == F32
        inside = (z > near) & (uf >= F32(0)) & (uf <= F32(W - 1)) & (vf >= F32(0)) & (vf <= F32(H - 1))
        uc = np.where(inside, uf, F32(0)).astype(np.int64)  # -0 -> 0
        vc = np.where(inside, vf, F32(0)).astype(np.int64)
        d = depth[vc, uc]
        tested = inside & (d > F32(0)) & (d < F32(np.inf))
        lo, hi = d * keep, d * beyond  # one rounded product each
        assert lo.dtype == F32 and hi.dtype == F32
        front, behind = tested & (z < lo), tested & (z > hi)
    return tested, tested & ~front & ~behind, front, behind


def score(means, w2cs, intr, depth, keep, beyond, near):
    """What gsl_map_score leaves in counts: int64 [k,3], per pose (rows tested, rows that agree, rows in front)."""
    w2cs = np.asarray(w2cs, dtype=F32).reshape(-1, 4, 4)
    out = np.zeros((len(w2cs), 3), dtype=np.int64)
    for k, w2c in enumerate(w2cs):
        tested, agree, front, _ = verdicts(means, w2c, intr, depth, keep, beyond, near)
        out[k] = tested.sum(), agree.sum(), front.sum()
    return out
