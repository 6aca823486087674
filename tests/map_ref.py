"""numpy mirror of csrc/map.hip: the selection rule, the raster-order compaction, the capacity clamp and the point /
colour arithmetic.  The rule is evaluated in float32, as the device evaluates it (one rounded product, comparisons); the
points and colours in float64 from the float32 inputs, with the rounding bound of the device's float32 chain beside
them."""
import numpy as np

F32 = np.float32
ULP = 2.0 ** -24  # half the spacing of float32 at 1: the relative error of one rounded operation


def keep_of(depth_rho):
    """keep = 1 - depth_rho, the float32 value the host computes."""
    return F32(1.0) - F32(depth_rho)


def select(d_o, d_r=None, a=None, alpha_min=0.5, keep=keep_of(0.05)):
    """[H,W] bool: d_o finite and > 0, and (a < alpha_min or d_o < d_r * keep).  d_r is None and a is None: the
    "no render yet" form, every valid pixel."""
    d_o = np.asarray(d_o, dtype=F32)
    with np.errstate(invalid="ignore"):
        new = np.isfinite(d_o) & (d_o > F32(0))
        if d_r is None and a is None:
            return new
        limit = np.asarray(d_r, dtype=F32) * F32(keep)  # float32 product, rounded once
        assert limit.dtype == F32
        return new & ((np.asarray(a, dtype=F32) < F32(alpha_min)) | (d_o < limit))


def clamp(selected, n_live, capacity):
    """Rows appended when ``selected`` rows are offered to a map with n_live of capacity rows live."""
    return int(min(selected, capacity - n_live))


def insert(d_o, rgb, intr, c2w, n_live, capacity, d_r=None, a=None, alpha_min=0.5, keep=keep_of(0.05)):
    """What the two entry points do to a map: dict with
       idx      flat raster indices (v * W + u) of the selected pixels, ascending,
       n_new    (selected, appended),
       means    [appended,3] float64 world points of the first ``appended`` selected pixels (rows n_live ...),
       colors   [appended,3] float64,
       bound    [appended,3] 8 * 2^-24 * (sum_k |R_jk| |p_k| + |t_j|): two divisions, three multiplications and the
                three-term sum of the device's float32 chain."""
    d_o = np.asarray(d_o, dtype=F32)
    H, W = d_o.shape
    idx = np.flatnonzero(select(d_o, d_r, a, alpha_min, keep).reshape(-1))
    appended = clamp(len(idx), n_live, capacity)
    kept = idx[:appended]
    fx, fy, cx, cy = (np.float64(F32(x)) for x in intr)
    c2w = np.asarray(c2w, dtype=F32).astype(np.float64).reshape(4, 4)
    u, v = (kept % W).astype(np.float64), (kept // W).astype(np.float64)
    d = d_o.reshape(-1)[kept].astype(np.float64)
    p = np.stack([(u - cx) / fx * d, (v - cy) / fy * d, d], axis=-1)  # depth_to_points
    R, t = c2w[:3, :3], c2w[:3, 3]
    means = p @ R.T + t
    bound = 8.0 * ULP * (np.abs(p) @ np.abs(R).T + np.abs(t))
    colors = np.asarray(rgb, dtype=F32).reshape(-1, 3)[kept].astype(np.float64) / 255.0
    return dict(idx=idx, n_new=(len(idx), appended), means=means, colors=colors, bound=bound)
