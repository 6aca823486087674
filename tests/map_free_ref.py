"""numpy mirror of csrc/map_free.hip: the free-space rule in float32, every operation rounded once in the device's order
(numpy's float32 multiply, add, divide and rint are the IEEE operations, and nothing here is fused), and the
ascending-order compaction of the rows that stay."""
import numpy as np

from tests.map_view_ref import w2c_of  # noqa: F401  (the pose the device is given is the local map's)

F32 = np.float32


def keep_of(free_rho):
    """keep = 1 - free_rho, the float32 value the host computes."""
    return F32(1.0) - F32(free_rho)


def rule(means, w2c, intr, depth, keep, window, near):
    """(kept [n] bool, tested [n] bool).  x = ((w0 px + w1 py) + w2 pz) + w3 (y, z likewise); u = fx x / z + cx,
    v = fy y / z + cy; uf = rint(u), vf = rint(v); tested = z > near and 0 <= uf <= W - 1 and 0 <= vf <= H - 1;
    blocked = some pixel of the (2 window + 1)^2 window around (uf, vf) inside the image has a depth d that is not
    (finite and > 0) or not (z < d * keep); kept = not (tested and not blocked)."""
    p = np.asarray(means, dtype=F32).reshape(-1, 3)
    w = np.asarray(w2c, dtype=F32).reshape(4, 4)
    depth = np.asarray(depth, dtype=F32)
    H, W = depth.shape
    fx, fy, cx, cy = (F32(a) for a in intr)
    keep, near, window = F32(keep), F32(near), int(window)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        x, y, z = (((w[j, 0] * px + w[j, 1] * py) + w[j, 2] * pz) + w[j, 3] for j in range(3))
        u, v = fx * x / z + cx, fy * y / z + cy
        uf, vf = np.rint(u), np.rint(v)  # round half to even
        assert uf.dtype == F32 and vf.dtype == F32 and z.dtype == F32
        tested = (z > near) & (uf >= F32(0)) & (uf <= F32(W - 1)) & (vf >= F32(0)) & (vf <= F32(H - 1))
        uc = np.where(tested, uf, F32(0)).astype(np.int64)  # -0 -> 0
        vc = np.where(tested, vf, F32(0)).astype(np.int64)
        limit = depth * keep  # one rounded product per pixel
        assert limit.dtype == F32
        valid = np.isfinite(depth) & (depth > F32(0))
        blocked = np.zeros(len(p), dtype=bool)
        for dv in range(-window, window + 1):
            for du in range(-window, window + 1):
                uu, vv = uc + du, vc + dv
                inside = (uu >= 0) & (uu <= W - 1) & (vv >= 0) & (vv <= H - 1)
                uu, vv = np.clip(uu, 0, W - 1), np.clip(vv, 0, H - 1)
                passes = valid[vv, uu] & (z < limit[vv, uu])
                blocked |= inside & ~passes
    return ~(tested & ~blocked), tested


def select(means, w2c, intr, depth, keep, window, near):
    """What gsl_map_free_select and gsl_map_view_gather leave: dict with
       kept      [n] bool, the rows that stay (the ballot bits),
       tested    [n] bool,
       ids       int32, the ascending old rows of the survivors,
       counters  (rows that stay, 0, rows stored) after the gather into a buffer with room for all of them."""
    kept, tested = rule(means, w2c, intr, depth, keep, window, near)
    ids = np.flatnonzero(kept).astype(np.int32)
    return dict(kept=kept, tested=tested, ids=ids, counters=(len(ids), 0, len(ids)))
