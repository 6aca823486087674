"""numpy mirror of csrc/map_place.hip and of the ranking of GaussianMap.match_place.

The descriptor: the image cut into GW x GH = 16 x 12 cells, pixel (u, v) in cell ((u * 16) // W, (v * 12) // H); a pixel
counts when d > 0 and d < inf; its value is q = uint32(rint(min(d, 63) * 1024)) -- one float32 product, numpy's rint is
round half to even as rintf is; a cell's value is sum(q) // count when count > 0 and 2 * count >= the cell's pixels,
else -1.  The match: per keyframe and shift (sx, sy) -- SHIFTS, sy-major, both ascending -- the cells (i, j) with
(i + sx, j + sy) inside the grid where query[j + sy][i + sx] and table[k][j][i] are both valid: their number and the sum
of the absolute differences.  The ranking: per keyframe the shift with the smallest sum / common among those with
common >= min_common, then the keyframes by that value; ties to the smaller |sx| + |sy|, the earlier shift, the lower
slot.  Fractions are exact (fractions.Fraction); everything else is integers."""
from fractions import Fraction

import numpy as np

F32 = np.float32
GW, GH = 16, 12
CELLS = GW * GH
SHIFTS = [(sx, sy) for sy in (-1, 0, 1) for sx in (-2, -1, 0, 1, 2)]
Q_MAX = 63 * 1024


def cell_of(u, v, W, H):
    """(ci, cj) of pixel (u, v)."""
    return (u * GW) // W, (v * GH) // H


def quantise(depth):
    """(counts, q): bool and uint32 arrays of the image's shape."""
    d = np.asarray(depth, dtype=F32)
    with np.errstate(all="ignore"):
        counts = (d > F32(0)) & (d < F32(np.inf))
        prod = np.minimum(np.where(counts, d, F32(0)), F32(63.0)) * F32(1024.0)
        assert prod.dtype == F32
        q = np.rint(prod).astype(np.uint32)
    return counts, np.where(counts, q, np.uint32(0))


def describe(depth):
    """int32 [192]: what gsl_map_place_describe leaves in desc."""
    d = np.asarray(depth, dtype=F32)
    H, W = d.shape
    assert W >= GW and H >= GH
    counts, q = quantise(d)
    ci = (np.arange(W, dtype=np.int64) * GW) // W
    cj = (np.arange(H, dtype=np.int64) * GH) // H
    cell = (cj[:, None] * GW + ci[None, :]).reshape(-1)
    total = np.bincount(cell, minlength=CELLS)
    count = np.bincount(cell[counts.reshape(-1)], minlength=CELLS)
    sums = np.zeros(CELLS, dtype=np.int64)
    np.add.at(sums, cell, q.reshape(-1).astype(np.int64))
    out = np.full(CELLS, -1, dtype=np.int32)
    ok = (count > 0) & (2 * count >= total)
    out[ok] = (sums[ok] // count[ok]).astype(np.int32)
    return out


def match(query, table):
    """int64 [n,15,2]: per keyframe and shift (common, sum), what gsl_map_place_match leaves in out."""
    q = np.asarray(query, dtype=np.int64).reshape(GH, GW)
    t = np.asarray(table, dtype=np.int64).reshape(-1, GH, GW)
    out = np.zeros((t.shape[0], len(SHIFTS), 2), dtype=np.int64)
    for s, (sx, sy) in enumerate(SHIFTS):
        i0, i1, j0, j1 = max(0, -sx), min(GW, GW - sx), max(0, -sy), min(GH, GH - sy)
        qs = q[j0 + sy:j1 + sy, i0 + sx:i1 + sx][None]
        ts = t[:, j0:j1, i0:i1]
        both = (qs >= 0) & (ts >= 0)
        out[:, s, 0] = both.sum(axis=(1, 2))
        out[:, s, 1] = (np.abs(qs - ts) * both).sum(axis=(1, 2))
    return out


def rank(result, min_common):
    """[(slot, sx, sy, sum, common), ...]: every keyframe's best admissible shift, the best keyframe first."""
    rows = []
    for slot, per_shift in enumerate(np.asarray(result).tolist()):
        best = None
        for s, (common, total) in enumerate(per_shift):
            if common < min_common or common == 0:
                continue
            sx, sy = SHIFTS[s]
            key = (Fraction(total, common), abs(sx) + abs(sy), s)
            if best is None or key < best[0]:
                best = (key, (slot, sx, sy, total, common))
        if best is not None:
            rows.append((best[0] + (slot,), best[1]))
    return [row for _, row in sorted(rows, key=lambda r: r[0])]
