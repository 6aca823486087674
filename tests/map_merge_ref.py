"""numpy mirror of csrc/map_merge.hip, the rule of include/gsloc_hip.h ("map resolution"): the float32 steps with
np.float32 (numpy's float32 multiply, subtract, floor and rint are the IEEE operations, and nothing here is fused), the
sums as integers in int64 / uint64, the doubles as written, and a stable order -- the voxels are found by sorting the
keys, which has nothing in common with the device's hash table."""
import numpy as np

F32 = np.float32
CELL_MAX = 2 ** 20 - 1


def h_of(merge_voxel):
    """(inv_h, h): the float32 values the host computes."""
    h = F32(merge_voxel)
    return F32(1.0) / h, h


def cells(means, inv_h):
    """(mergeable [n] bool, c [n,3] int64 -- 0 where a row is not mergeable, q [n,3] uint64 likewise, key [n] uint64)."""
    p = np.asarray(means, dtype=F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        f = p * F32(inv_h)  # one rounded product
        c = np.floor(f)
        assert f.dtype == F32 and c.dtype == F32
        ok = np.isfinite(f) & (np.abs(c) <= F32(CELL_MAX))  # per axis; false for a NaN
        mergeable = ok.all(axis=1)
        frac = (f - c) * F32(65536.0)
        assert frac.dtype == F32
        q = np.rint(frac)
    m3 = mergeable[:, None] & np.ones(3, dtype=bool)
    ci = np.where(m3, c, F32(0)).astype(np.int64)
    qi = np.where(m3, q, F32(0)).astype(np.uint64)
    b = (ci + CELL_MAX).astype(np.uint64)
    key = b[:, 0] | (b[:, 1] << np.uint64(21)) | (b[:, 2] << np.uint64(42))
    return mergeable, ci, qi, key


def colour_units(colors):
    """[n,3] uint64: rint(fmin(fmax(colour, 0), 1) * 65280); fmax gives the 0 for a NaN."""
    c = np.asarray(colors, dtype=F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        u = np.rint(np.fmin(np.fmax(c, F32(0)), F32(1)) * F32(65280.0))
    assert u.dtype == F32
    return u.astype(np.uint64)


def merge(means, colors, stamps, merge_voxel):
    """What gsl_map_merge_select, the two gathers and gsl_map_merge_apply leave: dict with
       kept      [n] bool, the rows that stay (the ballot bits),
       ids       int32, the ascending old rows of the survivors,
       means, colors [k,3] float32 and stamps [k] int32 of the survivors, fused where their voxel has more than one row,
       counters  (rows that stay, rows removed, rows stored, 0),
       k_of      [k] int64: the rows of each survivor's voxel (1 for a row that is not mergeable)."""
    means = np.ascontiguousarray(means, dtype=F32).reshape(-1, 3)
    colors = np.ascontiguousarray(colors, dtype=F32).reshape(-1, 3)
    stamps = np.ascontiguousarray(stamps, dtype=np.int32).reshape(-1)
    n = len(means)
    inv_h, h = h_of(merge_voxel)
    mergeable, c, q, key = cells(means, inv_h)
    cu = colour_units(colors)
    kept = np.ones(n, dtype=bool)
    out_m, out_c, out_s = means.copy(), colors.copy(), stamps.copy()
    k_of = np.ones(n, dtype=np.int64)
    rows = np.flatnonzero(mergeable)
    order = rows[np.argsort(key[rows], kind="stable")]  # voxel by voxel, ascending row inside a voxel
    if len(order):
        starts = np.flatnonzero(np.r_[True, key[order][1:] != key[order][:-1]])
        ends = np.r_[starts[1:], len(order)]
        for a, b in zip(starts, ends):
            if b - a == 1:
                continue
            members = order[a:b]
            first, k = int(members[0]), b - a
            assert first == members.min()
            kept[members[1:]] = False
            k_of[first] = k
            S = q[members].sum(axis=0, dtype=np.uint64)
            C = cu[members].sum(axis=0, dtype=np.uint64)
            for j in range(3):
                pos = (np.float64(c[first, j]) + np.float64(S[j]) / (np.float64(65536.0) * np.float64(k))) * np.float64(h)
                out_m[first, j] = F32(pos)
                out_c[first, j] = F32(np.float64(C[j]) / (np.float64(65280.0) * np.float64(k)))
            out_s[first] = stamps[members].max()
    ids = np.flatnonzero(kept).astype(np.int32)
    stay = len(ids)
    return dict(kept=kept, ids=ids, means=out_m[ids], colors=out_c[ids], stamps=out_s[ids],
                counters=(stay, n - stay, stay, 0), k_of=k_of[ids])


def occupancy(means, merge_voxel):
    """The largest number of mergeable rows in one voxel (0 for no mergeable row): 1 says nothing can be fused."""
    mergeable, _, _, key = cells(means, h_of(merge_voxel)[0])
    if not mergeable.any():
        return 0
    return int(np.unique(key[mergeable], return_counts=True)[1].max())
