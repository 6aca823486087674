"""numpy mirror of csrc/map_refine.hip: the rows a depth frame observes again move along their ray to the running mean
of their depths, in float32 with every operation rounded once in the device's order, one operation per line (numpy's
float32 multiply, add, subtract, divide and floor are the IEEE operations, and nothing here is fused).  The projection
is this file's own copy, as in the other tests/map_*_ref.py."""
import numpy as np

from tests.map_view_ref import w2c_of  # noqa: F401  (the float64 inverse rounded to float32: what the device is given)

F32 = np.float32


def keep_of(rho):
    """keep = 1 - rho, the float32 value the host computes."""
    return F32(1.0) - F32(rho)


def cam_of(c2w):
    """The camera centre the device is given: the translation of the pose, rounded to float32."""
    return np.asarray(c2w, dtype=np.float64).reshape(4, 4)[:3, 3].astype(F32)


def project(means, w2c, intr):
    """(z, u, v), float32 [n] each: x = ((w0 px + w1 py) + w2 pz) + w3 (y, z likewise); u = fx x / z + cx,
    v = fy y / z + cy."""
    p = np.asarray(means, dtype=F32).reshape(-1, 3)
    w = np.asarray(w2c, dtype=F32).reshape(4, 4)
    fx, fy, cx, cy = (F32(a) for a in intr)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        x, y, z = (((w[j, 0] * px + w[j, 1] * py) + w[j, 2] * pz) + w[j, 3] for j in range(3))
        u, v = fx * x / z + cx, fy * y / z + cy
    assert u.dtype == F32 and v.dtype == F32 and z.dtype == F32
    return z, u, v


def _blend(k, x00, x10, x01, x11):
    """((w00 x00 + w10 x10) + w01 x01) + w11 x11, left to right."""
    s = k[0] * x00
    t = k[1] * x10
    s = s + t
    t = k[2] * x01
    s = s + t
    t = k[3] * x11
    s = s + t
    assert s.dtype == F32
    return s


def nearest_depth(depth, u, v):
    """The plain alternative to the blend that the rule does NOT use: the depth of the pixel nearest to (u, v)."""
    H, W = depth.shape
    return depth[np.clip(np.rint(v), 0, H - 1).astype(np.int64), np.clip(np.rint(u), 0, W - 1).astype(np.int64)]


def refine(means, colors, weights, w2c, cam, intr, depth, rgb, keep, near, max_weight, observed=None):
    """What gsl_map_refine leaves: dict with
       means    float32 [n,3], colors float32 [n,3] (the input's bits when rgb is None), weights int32 [n],
       refined  bool [n], count = refined.sum() (counters[0]),
       a, b     float32 [n]: the position inside the four pixels (of every row, refined or not),
       d        float32 [n]: the observed depth on the row's ray (of the refined rows; elsewhere unspecified).
    observed(depth, u, v) -> float32 [n]: another observed depth in place of the inverse-depth blend (the tests hold
    the nearest-pixel read against it); the device has no such thing."""
    p = np.array(means, dtype=F32).reshape(-1, 3)
    c = None if colors is None else np.array(colors, dtype=F32).reshape(-1, 3)
    w = np.array(weights, dtype=np.int32).reshape(-1)
    depth = np.asarray(depth, dtype=F32)
    H, W = depth.shape
    assert W >= 2 and H >= 2 and 1 <= int(max_weight) <= 2 ** 30
    keep, near = F32(keep), F32(near)
    cam = np.asarray(cam, dtype=F32).reshape(3)
    z, u, v = project(p, w2c, intr)
    with np.errstate(all="ignore"):
        cand = (z > near) & (u >= F32(0)) & (u <= F32(W - 1)) & (v >= F32(0)) & (v <= F32(H - 1))
        us, vs = np.where(cand, u, F32(0)), np.where(cand, v, F32(0))
        u0 = np.minimum(np.floor(us).astype(np.int64), W - 2)
        v0 = np.minimum(np.floor(vs).astype(np.int64), H - 2)
        a = u - u0.astype(F32)
        b = v - v0.astype(F32)
        d00, d10, d01, d11 = depth[v0, u0], depth[v0, u0 + 1], depth[v0 + 1, u0], depth[v0 + 1, u0 + 1]
        zk = z * keep
        refined = cand.copy()
        for d in (d00, d10, d01, d11):
            lo = d * keep
            refined &= (d > F32(0)) & (d < F32(np.inf)) & (z >= lo) & (zk <= d)
        a1 = F32(1) - a
        b1 = F32(1) - b
        k = (a1 * b1, a * b1, a1 * b, a * b)
        if observed is None:
            q = _blend(k, F32(1) / d00, F32(1) / d10, F32(1) / d01, F32(1) / d11)
            d = F32(1) / q
        else:
            d = np.asarray(observed(depth, us, vs), dtype=F32)
        w1 = w.astype(np.int64) + 1
        wf = w1.astype(F32)
        num = d - z
        den = z * wf
        t = num / den
        out_p = p.copy()
        for j in range(3):
            ray = p[:, j] - cam[j]
            step = ray * t
            moved = p[:, j] + step
            assert moved.dtype == F32
            out_p[:, j] = np.where(refined, moved, p[:, j])
        out_c = c
        if rgb is not None:
            rgb = np.asarray(rgb, dtype=F32).reshape(H, W, 3)
            out_c = c.copy()
            for j in range(3):
                ch = rgb[:, :, j] / F32(255)
                s = _blend(k, ch[v0, u0], ch[v0, u0 + 1], ch[v0 + 1, u0], ch[v0 + 1, u0 + 1])
                diff = s - c[:, j]
                gain = diff / wf
                moved = c[:, j] + gain
                assert moved.dtype == F32
                out_c[:, j] = np.where(refined, moved, c[:, j])
        out_w = np.where(refined, np.minimum(w1, int(max_weight)), w).astype(np.int32)
    return dict(means=out_p, colors=out_c, weights=out_w, refined=refined, count=int(refined.sum()), a=a, b=b, d=d)
