"""numpy mirror of csrc/map_occl.hip: the band rule and the projection in float32, every operation rounded once in the
device's order (its own copy, on purpose: tests/map_view_ref.py has another), the z-buffer of complemented depth bits per
cell, the window minimum, the occlusion verdict, the ascending-order compaction with its capacity clamp and the four
counters."""
import numpy as np

F32 = np.float32
CELLS = (1, 2, 4, 8, 16)


def w2c_of(c2w):
    """The float64 inverse of a camera-to-world pose, rounded to float32: what GaussianMap hands to the device."""
    return np.linalg.inv(np.asarray(c2w, dtype=np.float64).reshape(4, 4)).astype(F32)


def keep_of(rho):
    """1 - rho as the host takes it: the float32 difference of the float32 values."""
    return F32(1.0) - F32(rho)


def project(means, w2c, intr):
    """(z, u, v) float32 [n]: x = ((w0 px + w1 py) + w2 pz) + w3 (y, z likewise); u = fx x / z + cx, v = fy y / z + cy."""
    p = np.asarray(means, dtype=F32).reshape(-1, 3)
    w = np.asarray(w2c, dtype=F32).reshape(4, 4)
    fx, fy, cx, cy = (F32(a) for a in intr)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        x, y, z = (((w[j, 0] * px + w[j, 1] * py) + w[j, 2] * pz) + w[j, 3] for j in range(3))
        u, v = fx * x / z + cx, fy * y / z + cy
    assert u.dtype == F32 and v.dtype == F32 and z.dtype == F32
    return z, u, v


def in_band(z, u, v, width, height, guard_px, near, far):
    g, near, far = F32(guard_px), F32(near), F32(far)
    u_hi, v_hi = F32(width - 1) + g, F32(height - 1) + g
    with np.errstate(all="ignore"):
        return (z > near) & (z < far) & (u >= -g) & (u <= u_hi) & (v >= -g) & (v <= v_hi)


def grid(width, height, guard_px, cell_px):
    """(gi, CH, CW)."""
    assert cell_px in CELLS and guard_px >= 0
    gi = int(np.ceil(F32(guard_px)))
    return gi, (height - 1 + 2 * gi) // cell_px + 1, (width - 1 + 2 * gi) // cell_px + 1


def cells(u, v, band, gi, cell_px):
    """(cu, cv) int64 [n]; -1 where the row is not in the band."""
    inv = F32(1.0) / F32(cell_px)
    cu, cv = np.full(u.shape, -1, np.int64), np.full(u.shape, -1, np.int64)
    cu[band] = np.floor((u[band] + F32(gi)) * inv).astype(np.int64)
    cv[band] = np.floor((v[band] + F32(gi)) * inv).astype(np.int64)
    return cu, cv


def _state(means, w2c, intr, width, height, guard_px, cell_px, near, far):
    assert near >= 0
    z, u, v = project(means, w2c, intr)
    band = in_band(z, u, v, width, height, guard_px, near, far)
    gi, ch, cw = grid(width, height, guard_px, cell_px)
    cu, cv = cells(u, v, band, gi, cell_px)
    assert (cu[band] >= 0).all() and (cu[band] < cw).all() and (cv[band] >= 0).all() and (cv[band] < ch).all()
    return z, band, cu, cv, ch, cw


def zbuf(means, w2c, intr, width, height, guard_px, cell_px, near, far):
    """uint32 [CH, CW]: 0 where no row in the band falls into the cell, else the maximum of ~bits(z) over them."""
    z, band, cu, cv, ch, cw = _state(means, w2c, intr, width, height, guard_px, cell_px, near, far)
    buf = np.zeros(ch * cw, np.uint32)
    keys = ~np.ascontiguousarray(z[band]).view(np.uint32)
    assert (keys != 0).all()
    np.maximum.at(buf, cv[band] * cw + cu[band], keys)
    return buf.reshape(ch, cw)


def depth_of(zb):
    """float32 [CH, CW]: the nearest depth per cell, inf where the cell is empty."""
    out = (~zb).view(F32).copy()
    out[zb == 0] = np.inf
    return out


def select(means, w2c, intr, width, height, guard_px, near, far, cell_px=4, window=1, rho=0.05, out_capacity=None,
           prev=None, zb=None):
    """What gsl_map_occl_depth (unless ``zb`` is given), gsl_map_occl_select and gsl_map_view_gather leave: dict with
       zbuf      uint32 [CH, CW],
       band      [n] bool, the rows in the band,
       culled    [n] bool, the rows in the band that are occluded,
       mask      [n] bool, the rows selected: in the band and not occluded,
       ids       the ascending indices of the rows written (the first ``out_capacity`` selected ones),
       counters  (selected, selected whose bit is clear in ``prev`` -- 0 without one --, written, culled)."""
    assert 0 <= window <= 3 and 0.0 < rho < 1.0
    z, band, cu, cv, ch, cw = _state(means, w2c, intr, width, height, guard_px, cell_px, near, far)
    if zb is None:
        zb = zbuf(means, w2c, intr, width, height, guard_px, cell_px, near, far)
    assert zb.shape == (ch, cw) and zb.dtype == np.uint32
    pad = np.zeros((ch + 2 * window, cw + 2 * window), np.uint32)  # a cell outside the grid counts as 0
    pad[window:window + ch, window:window + cw] = zb
    b_cu, b_cv, b_z = cu[band], cv[band], z[band]
    m = np.full(b_z.shape, 0xFFFFFFFF, np.uint32)
    for dv in range(-window, window + 1):
        for du in range(-window, window + 1):
            m = np.minimum(m, pad[b_cv + window + dv, b_cu + window + du])
    with np.errstate(all="ignore"):
        product = keep_of(rho) * b_z
        assert product.dtype == F32
        occluded = (m != 0) & (product > (~m).view(F32))
    culled = np.zeros(band.shape, bool)
    culled[band] = occluded
    mask = band & ~culled
    ids = np.flatnonzero(mask)
    written = len(ids) if out_capacity is None else min(len(ids), int(out_capacity))
    fresh = 0 if prev is None else int((mask & ~np.asarray(prev, dtype=bool)).sum())
    return dict(zbuf=zb, band=band, culled=culled, mask=mask, ids=ids[:written].astype(np.int32),
                counters=(len(ids), fresh, written, int(culled.sum())))


def violations(means, w2c, intr, width, height, reach_px, near, far, cell_px, window, rho, prev):
    """Rows VISIBLE from this pose -- in the band of the reach and not occluded in the z-buffer built there -- that the
    earlier selection ``prev`` ([n] bool) left out.  A row parallax has uncovered counts; a row occluded from both poses
    does not."""
    return select(means, w2c, intr, width, height, reach_px, near, far, cell_px, window, rho, prev=prev)["counters"][1]
