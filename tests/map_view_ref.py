"""numpy mirror of csrc/map_view.hip: the in-view rule in float32, every operation rounded once in the device's order
(numpy's float32 multiply, add and divide are the IEEE operations, and nothing here is fused), the ascending-order
compaction with its capacity clamp, and the violation count in_view_now & ~in_view_prev."""
import numpy as np

F32 = np.float32


def w2c_of(c2w):
    """The float64 inverse of a camera-to-world pose, rounded to float32: what GaussianMap hands to the device."""
    return np.linalg.inv(np.asarray(c2w, dtype=np.float64).reshape(4, 4)).astype(F32)


def in_view(means, w2c, intr, width, height, guard_px, near, far):
    """[n] bool.  x = ((w0 px + w1 py) + w2 pz) + w3 (y, z likewise); z > near and z < far; u = fx x / z + cx,
    v = fy y / z + cy; -guard <= u <= (width - 1) + guard, -guard <= v <= (height - 1) + guard."""
    p = np.asarray(means, dtype=F32).reshape(-1, 3)
    w = np.asarray(w2c, dtype=F32).reshape(4, 4)
    fx, fy, cx, cy = (F32(a) for a in intr)
    g, near, far = F32(guard_px), F32(near), F32(far)
    u_hi, v_hi = F32(width - 1) + g, F32(height - 1) + g
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        x, y, z = (((w[j, 0] * px + w[j, 1] * py) + w[j, 2] * pz) + w[j, 3] for j in range(3))
        u, v = fx * x / z + cx, fy * y / z + cy
        assert u.dtype == F32 and v.dtype == F32 and z.dtype == F32
        return (z > near) & (z < far) & (u >= -g) & (u <= u_hi) & (v >= -g) & (v <= v_hi)


def select(means, w2c, intr, width, height, guard_px, near, far, out_capacity=None, prev=None):
    """What the two entry points leave: dict with
       mask      [n] bool, the rows in view,
       ids       the ascending indices of the rows written (the first ``out_capacity`` selected ones),
       counters  (rows in view, rows in view whose bit is clear in ``prev`` -- 0 without one --, rows written)."""
    mask = in_view(means, w2c, intr, width, height, guard_px, near, far)
    ids = np.flatnonzero(mask)
    written = len(ids) if out_capacity is None else min(len(ids), int(out_capacity))
    fresh = 0 if prev is None else int((mask & ~np.asarray(prev, dtype=bool)).sum())
    return dict(mask=mask, ids=ids[:written].astype(np.int32), counters=(len(ids), fresh, written))


def violations(means, w2c, intr, width, height, reach_px, near, far, prev):
    """Rows in view at this pose with the reach as guard that the earlier selection ``prev`` ([n] bool) left out."""
    return select(means, w2c, intr, width, height, reach_px, near, far, prev=prev)["counters"][1]
