"""numpy mirror of csrc/map_exposure.hip: the seven integers of k_map_exposure_sums, the float64 solve of
k_map_exposure_solve, the launch sequence of gsl_map_exposure_estimate and the correction of gsl_map_exposure_apply --
float32 (the solve: float64) with every operation rounded once in the device's order; numpy's multiply, add, subtract,
divide and rint are the IEEE operations and nothing here is fused.  Its own copy of the projection rule, as the other
mirrors have on purpose."""
import numpy as np

F32, F64 = np.float32, np.float64
VALUES, RECORD_WORDS, MAX_PASSES = 7, 6, 4
OK, FEW, FLAT, RANGE = 0, 1, 2, 3
NAMES = ["OK", "FEW", "FLAT", "RANGE"]
ONE = F32(1048576.0)  # 2^20
WR, WG, WB = F32(0.299), F32(0.587), F32(0.114)
IDENTITY = np.array([1.0, 0.0, 0.0, 0.0], F32)
# MapConfig's defaults, in the order of estimate(): sat_lo, sat_hi, max_residual, passes, min_used, gain_min, gain_max,
# offset_max, min_var
DEFAULTS = (F32(0.02), F32(0.98), F32(0.1), 2, 256, 0.5, 2.0, 0.25, 1e-4)


def rows(means, colors, w2c, intr, depth, image, keep, beyond, near, sat_lo, sat_hi, gate, params):
    """(seen [n], used [n], Y0 [n], Yi [n] float32; Y0 is garbage where the row is not seen)."""
    p = np.asarray(means, dtype=F32).reshape(-1, 3)
    col = np.asarray(colors, dtype=F32).reshape(-1, 3)
    w = np.asarray(w2c, dtype=F32).reshape(4, 4)
    depth, Y = np.asarray(depth, dtype=F32), np.asarray(image, dtype=F32)
    H, W = depth.shape
    assert Y.shape == depth.shape and len(col) == len(p)
    fx, fy, cx, cy = (F32(a) for a in intr)
    keep, beyond, near = F32(keep), F32(beyond), F32(near)
    lo, hi, gate = F32(sat_lo), F32(sat_hi), F32(gate)
    g0, b0 = F32(params[0]), F32(params[1])
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    zero = F32(0)
    with np.errstate(all="ignore"):
        x, y, z = (((w[j, 0] * px + w[j, 1] * py) + w[j, 2] * pz) + w[j, 3] for j in range(3))
        u, v = fx * x / z + cx, fy * y / z + cy
        uf, vf = np.rint(u), np.rint(v)  # round half to even
        inside = (z > near) & (uf >= zero) & (uf <= F32(W - 1)) & (vf >= zero) & (vf <= F32(H - 1))
        uc = np.where(inside, uf, zero).astype(np.int64)
        vc = np.where(inside, vf, zero).astype(np.int64)
        d0 = depth[vc, uc]
        seen = inside & (d0 > zero) & (d0 < F32(np.inf)) & (d0 * keep <= z) & (z <= d0 * beyond)
        Yi = (WR * col[:, 0] + WG * col[:, 1]) + WB * col[:, 2]
        Y0 = Y[vc, uc]
        used = seen & (Yi >= lo) & (Yi <= hi) & (Y0 >= lo) & (Y0 <= hi)
        used &= np.abs((g0 * Y0 + b0) - Yi) <= gate
        assert Yi.dtype == F32 and Y0.dtype == F32 and z.dtype == F32
    return seen, used, Y0, Yi


def fixed(s, t):
    with np.errstate(all="ignore"):
        scaled = (s * t) * ONE  # one float32 product, then an exact scaling
    assert scaled.dtype == F32
    return int(np.rint(scaled).astype(np.int64).sum())  # round half to even


def sums(means, colors, w2c, intr, depth, image, keep, beyond, near, sat_lo, sat_hi, gate, params):
    """What k_map_exposure_sums leaves: int64 [7]."""
    seen, used, Y0, Yi = rows(means, colors, w2c, intr, depth, image, keep, beyond, near, sat_lo, sat_hi, gate, params)
    x, y, one = Y0[used], Yi[used], np.ones(int(used.sum()), F32)
    return np.array([fixed(x, x), fixed(x, one), fixed(x, y), fixed(y, one), fixed(y, y), used.sum(), seen.sum()],
                    dtype=np.int64)


def solve(out, k, params, record, min_used, gain_min, gain_max, offset_max, min_var):
    """k_map_exposure_solve: params float32 [4] and record [passes] of (status, used, seen, g, b, rss), in place."""
    out = np.asarray(out, dtype=np.int64)
    used, seen = int(out[5]), int(out[6])
    one = F64(1048576.0)
    n = F64(used)
    Sxx, Sx, Sxy, Sy, Syy = (F64(int(a)) / one for a in out[:5])
    status, g, b, rss = OK, F64(params[0]), F64(params[1]), F64(0.0)
    with np.errstate(all="ignore"):
        if k > 0 and record[k - 1][0] != OK:
            status = record[k - 1][0]
        elif used < min_used:
            status = FEW
        else:
            det = n * Sxx - Sx * Sx
            if not (det / (n * n) > F64(min_var)):
                status = FLAT
            else:
                g = (n * Sxy - Sx * Sy) / det
                b = (Sy - g * Sx) / n
                rss = (Syy - g * Sxy) - b * Sy
                if not (F64(gain_min) <= g <= F64(gain_max) and abs(b) <= F64(offset_max)):
                    status = RANGE
                else:
                    bf = F32(b)
                    params[0], params[1], params[2], params[3] = F32(g), bf, bf * F32(255.0), F32(0)
    record[k] = (int(status), used, seen, float(g), float(b), float(rss))


def estimate(means, colors, w2c, intr, depth, image, keep, beyond, near, sat_lo, sat_hi, max_residual, passes, min_used,
             gain_min, gain_max, offset_max, min_var):
    """What gsl_map_exposure_estimate leaves: (sums int64 [7] of the last pass, params float32 [4], record [passes] of
    (status, used, seen, g, b, rss))."""
    assert 1 <= passes <= MAX_PASSES
    params = IDENTITY.copy()
    record, out = [None] * passes, None
    for k in range(passes):
        gate = F32(np.inf) if k == 0 else F32(max_residual)
        out = sums(means, colors, w2c, intr, depth, image, keep, beyond, near, sat_lo, sat_hi, gate, params)
        solve(out, k, params, record, min_used, gain_min, gain_max, offset_max, min_var)
    return out, params, record


def record_words(record):
    """The record as the device stores it: int64 [passes, 6], the doubles by their bits."""
    out = np.zeros((len(record), RECORD_WORDS), np.int64)
    for k, r in enumerate(record):
        out[k, :3] = r[:3]
        out[k, 3:] = np.array(r[3:], F64).view(np.int64)
    return out


def apply(rgb, params):
    """gsl_map_exposure_apply: float32, the shape of rgb."""
    c = np.asarray(rgb, dtype=F32)
    with np.errstate(all="ignore"):
        t = (F32(params[0]) * c) + F32(params[2])
        out = np.where(t < F32(0), F32(0), np.where(t > F32(255), F32(255), t))
    assert out.dtype == F32
    return out


def params_of(gain, offset):
    """params float32 [4] of a (gain, offset) pair, as the host uploads it."""
    b = F32(offset)
    return np.array([F32(gain), b, b * F32(255.0), 0.0], F32)
