"""numpy mirror of csrc/map_evict.hip: the OBSERVED rule in float32, every operation rounded once in the device's order
(numpy's float32 multiply, add, divide and rint are the IEEE operations, and nothing here is fused), and the eviction
rule, which is integers only: ages, the threshold age a*, the tie quota, and the ascending-order compaction of the rows
that stay."""
import numpy as np

from tests.map_view_ref import w2c_of  # noqa: F401  (the pose the device is given is the local map's)

F32 = np.float32
AGE_MAX = 1023


def keep_of(depth_rho):
    """keep = 1 - depth_rho, the float32 value the host computes."""
    return F32(1.0) - F32(depth_rho)


def observed(means, w2c, intr, depth, keep, window, reach, near, far):
    """[n] bool.  x = ((w0 px + w1 py) + w2 pz) + w3 (y, z likewise); u = fx x / z + cx, v = fy y / z + cy; uf = rint(u),
    vf = rint(v); in reach = z > near and z < far and -reach <= u <= (W - 1) + reach (v likewise); inside = 0 <= uf <=
    W - 1 and 0 <= vf <= H - 1; agrees = some pixel of the (2 window + 1)^2 window around (uf, vf) inside the image has a
    depth d, finite and > 0, with z >= d * keep and z * keep <= d; observed = in reach and (not inside or agrees)."""
    p = np.asarray(means, dtype=F32).reshape(-1, 3)
    w = np.asarray(w2c, dtype=F32).reshape(4, 4)
    depth = np.asarray(depth, dtype=F32)
    H, W = depth.shape
    fx, fy, cx, cy = (F32(a) for a in intr)
    keep, near, far, g, window = F32(keep), F32(near), F32(far), F32(reach), int(window)
    u_hi, v_hi = F32(W - 1) + g, F32(H - 1) + g
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        x, y, z = (((w[j, 0] * px + w[j, 1] * py) + w[j, 2] * pz) + w[j, 3] for j in range(3))
        u, v = fx * x / z + cx, fy * y / z + cy
        uf, vf = np.rint(u), np.rint(v)  # round half to even
        assert uf.dtype == F32 and vf.dtype == F32 and z.dtype == F32
        in_reach = (z > near) & (z < far) & (u >= -g) & (u <= u_hi) & (v >= -g) & (v <= v_hi)
        inside = (uf >= F32(0)) & (uf <= F32(W - 1)) & (vf >= F32(0)) & (vf <= F32(H - 1))
        uc = np.where(inside, uf, F32(0)).astype(np.int64)  # -0 -> 0
        vc = np.where(inside, vf, F32(0)).astype(np.int64)
        limit = depth * keep  # one rounded product per pixel
        zk = z * keep  # and one per row
        assert limit.dtype == F32 and zk.dtype == F32
        valid = np.isfinite(depth) & (depth > F32(0))
        agrees = np.zeros(len(p), dtype=bool)
        for dv in range(-window, window + 1):
            for du in range(-window, window + 1):
                uu, vv = uc + du, vc + dv
                ok = (uu >= 0) & (uu <= W - 1) & (vv >= 0) & (vv <= H - 1)
                uu, vv = np.clip(uu, 0, W - 1), np.clip(vv, 0, H - 1)
                agrees |= ok & valid[vv, uu] & (z >= limit[vv, uu]) & (zk <= depth[vv, uu])
    return in_reach & (~inside | agrees)


def stamp(stamps, seen, now):
    """The stamps after gsl_map_observe: ``now`` where ``seen``, the old stamp elsewhere."""
    return np.where(seen, np.int32(now), np.asarray(stamps, dtype=np.int32)).astype(np.int32)


def ages(stamps, now):
    """clamp(now - stamp, 0, 1023), the difference in 64 bits."""
    return np.clip(np.int64(now) - np.asarray(stamps, dtype=np.int32).astype(np.int64), 0, AGE_MAX)


def select(stamps, now, min_age, need):
    """What gsl_map_evict_select and gsl_map_view_gather leave: dict with
       kept      [n] bool, the rows that stay (the ballot bits),
       ties      [n] bool, the rows of age a* (the second ballot set),
       ids       int32, the ascending old rows of the survivors,
       counters  (rows that stay, E, rows stored) after the gather into a buffer with room for all of them,
       a_star, quota, E, evictable."""
    age = ages(stamps, now)
    n, need, min_age = len(age), int(need), int(min_age)
    assert need >= 0 and min_age >= 1
    evictable = int((age >= min_age).sum())
    E = min(need, evictable)
    at_least = np.cumsum(np.bincount(age, minlength=AGE_MAX + 1)[::-1])[::-1]  # at_least[a]: rows with age >= a
    a_star = int(np.flatnonzero(at_least >= E).max())
    older = int((age > a_star).sum())
    quota = E - older
    ties = age == a_star
    rank = np.cumsum(ties) - 1  # among the ties, in map order
    goes = (age > a_star) | (ties & (rank < quota))
    assert int(goes.sum()) == E and 0 <= quota <= int(ties.sum())
    ids = np.flatnonzero(~goes).astype(np.int32)
    return dict(kept=~goes, ties=ties, ids=ids, counters=(n - E, E, n - E), a_star=a_star, quota=quota, E=E,
                evictable=evictable)
