"""GPU: gsl_map_merge_select (csrc/map_merge.hip), gsl_map_view_gather, gsl_map_gather_i32 and gsl_map_merge_apply against
the numpy mirror tests/map_merge_ref.py on given arrays, and GaussianMap.merge.

Row counts: 1; 63 / 64 / 65 around one wave; 255 / 256 / 257 around one workgroup; 1000; 4099 (17 workgroups, three rows
in the last).  Patterns: every row its own voxel; all rows in one voxel; pairs adjacent in map order; pairs (i, i + n / 2)
-- from 1000 rows on the partners lie in different workgroups, and the first row of a pair sits between its neighbours'
partners; pairs and triples dealt at random over the map; a random cloud at about 3 rows per voxel (the table probes);
rows on voxel faces at positive and negative coordinates (h = 0.25, every coordinate a multiple of it); the cloud with
NaN / inf / out-of-range rows sprinkled in.  Colours: 8-bit values, or values from -0.5 to 1.5 with NaNs.  Stamps random.

Every case asserts: the counters after the selection and at the end; the ballots of the rows that stay; out_ids strictly
ascending and the mirror's; means, colours and stamps equal to the mirror's IN EVERY BIT; the sentinel rows past the
count, a guard region behind the outputs and the bytes behind the workspace untouched; the inputs unchanged; and a second
run on the same inputs, into a fresh workspace, equal to the first in every bit."""
import numpy as np
import pytest
import torch

from gsplatloc_amd import _lib
from gsplatloc_amd.mapping import GaussianMap, MapConfig
from tests import map_merge_ref as ref
from tests.test_gpu_map_view import GUARD_ROWS, H, SENTINEL, W

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
ROWS = [1, 63, 64, 65, 255, 256, 257, 1000, 4099]
PATTERNS = ["own", "one", "adjacent", "halves", "dealt", "cloud", "faces", "special"]
BAD_ARG, WORKSPACE = -1, -2  # GSL_ERR_BAD_ARG, GSL_ERR_WORKSPACE


def _case(n, pattern):
    """(means [n,3], colors [n,3], stamps [n], merge_voxel)."""
    rng = np.random.default_rng(1000 * n + len(pattern))
    i = np.arange(n)
    h = 0.25 if pattern == "faces" else 0.07
    inside = rng.uniform(0.05, 0.95, (n, 3))  # where in its voxel a row lies, in voxels

    def at(voxel):  # voxel [n] -> a cell per voxel, spread over the three axes and both signs
        cell = np.stack([voxel % 23 - 11, (voxel // 23) % 19 - 9, voxel // (23 * 19) - 4], axis=-1)
        return (cell + inside) * h

    if pattern == "own":
        means = at(i)
    elif pattern == "one":
        means = at(np.full(n, 777))
    elif pattern == "adjacent":
        means = at(i // 2)
    elif pattern == "halves":
        means = at(i % max(n // 2, 1))
    elif pattern == "dealt":
        means = at(rng.permutation(n) * 2 // 5)  # voxels of 2 and 3 rows, anywhere in the map
    elif pattern == "faces":
        means = rng.integers(-6, 7, (n, 3)) * h  # at most 13^3 voxels, every row on three faces
        means[rng.random(n) < 0.2] *= 0.0  # a heap at the origin, some of it -0.0
        means[rng.random(n) < 0.1] *= -1.0
    else:
        side = max(n / 3.0, 1.0) ** (1.0 / 3.0) * h
        means = rng.uniform(-side / 2, side / 2, (n, 3))
    means = means.astype(F32)
    if pattern == "special":
        far = float(F32(2 ** 20) * F32(h))
        for value in (np.nan, np.inf, -np.inf, far, -far - 1.0, 3.0e38):
            where = rng.random(n) < 0.04
            means[where, rng.integers(0, 3)] = value
    if pattern in ("own", "adjacent", "cloud", "faces"):
        colors = rng.integers(0, 256, (n, 3)).astype(F32) / F32(255.0)
    else:
        colors = rng.uniform(-0.5, 1.5, (n, 3)).astype(F32)
        colors[rng.random((n, 3)) < 0.05] = np.nan
    stamps = rng.integers(-5, 3000, n).astype(np.int32)
    return means, colors, stamps, h


def _bits(words, n):
    bits = ((words[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool).reshape(-1)
    assert not bits[n:].any()  # lanes past the last row hold nothing
    return bits[:n]


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _run(means, colors, stamps, h):
    """The four entry points on outputs of n + 3 + GUARD_ROWS sentinel rows; everything that was written, on the host."""
    lib, ptr, st = _lib.load_library(), _lib.ptr, _lib.current_stream()
    n = len(stamps)
    inv_h, h32 = ref.h_of(h)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    m_t, c_t, s_t = t(means), t(colors), t(stamps)
    rows = n + 3 + GUARD_ROWS
    out_m = torch.full((rows, 3), SENTINEL, device=DEV)
    out_c = torch.full((rows, 3), SENTINEL, device=DEV)
    out_i = torch.full((rows,), -77, dtype=torch.int32, device=DEV)
    out_s = torch.full((rows,), -88, dtype=torch.int32, device=DEV)
    counters = torch.full((4,), -5, dtype=torch.int32, device=DEV)
    ws_bytes = lib.gsl_map_merge_ws_bytes(n)
    ws = torch.full((ws_bytes + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    _lib.check(lib.gsl_map_merge_select(ptr(m_t), ptr(c_t), ptr(s_t), n, float(inv_h), float(h32), ptr(counters), ptr(ws),
                                        ws_bytes, st), "gsl_map_merge_select")
    first = counters.tolist()
    _lib.check(lib.gsl_map_view_gather(ptr(m_t), ptr(c_t), n, ptr(out_m), ptr(out_c), ptr(out_i), n + 3, ptr(counters),
                                       ptr(ws), ws_bytes, st), "gsl_map_view_gather")
    second = counters.tolist()
    _lib.check(lib.gsl_map_gather_i32(ptr(s_t), n, ptr(out_i), second[2], ptr(out_s), st), "gsl_map_gather_i32")
    _lib.check(lib.gsl_map_merge_apply(ptr(out_i), ptr(counters), n, ptr(out_m), ptr(out_c), ptr(out_s), ptr(ws),
                                       ws_bytes, st), "gsl_map_merge_apply")
    torch.cuda.synchronize()
    assert bool((ws[ws_bytes:] == 0xAB).all())  # nothing behind the size the library asked for
    for dev, host in ((m_t, means), (c_t, colors), (s_t, stamps)):  # the inputs are only read
        assert np.array_equal(_u32(dev.cpu().numpy()), _u32(host))
    nb = (n + 255) // 256
    raw = ws[:ws_bytes].cpu().numpy()
    return dict(first=first, second=second, counters=counters.tolist(), kept=_bits(raw[:32 * nb].view(np.uint64), n),
                ids=out_i.cpu().numpy(), means=out_m.cpu().numpy(), colors=out_c.cpu().numpy(), stamps=out_s.cpu().numpy())


def _check(got, want, n):
    k, removed = len(want["ids"]), n - len(want["ids"])
    assert got["first"] == [k, removed, 0, 0]  # after the selection: rows that stay, rows removed, nothing gathered
    assert got["second"] == [k, removed, k, 0] and tuple(got["counters"]) == want["counters"] == (k, removed, k, 0)
    assert np.array_equal(got["kept"], want["kept"])
    assert np.array_equal(got["ids"][:k], want["ids"]) and (np.diff(got["ids"][:k]) > 0).all()
    for name in ("means", "colors", "stamps"):
        same = _u32(got[name][:k]) == _u32(want[name])
        assert same.all(), (name, np.argwhere(~same)[:5].tolist())
    assert (got["ids"][k:] == -77).all() and (got["stamps"][k:] == -88).all()
    assert (got["means"][k:] == SENTINEL).all() and (got["colors"][k:] == SENTINEL).all()
    assert got["ids"].shape[0] == n + 3 + GUARD_ROWS


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", ROWS)
def test_the_entry_points_against_the_mirror(n, pattern):
    means, colors, stamps, h = _case(n, pattern)
    want = ref.merge(means, colors, stamps, h)
    removed = n - len(want["ids"])
    # the case is what it says
    if pattern == "own":
        assert removed == 0
    elif pattern == "one":
        assert removed == n - 1
    elif pattern == "adjacent":
        assert removed == n // 2
    elif pattern == "halves":
        assert removed == n - max(n // 2, 1)  # an odd n: its last row is a third row of voxel 0
    elif pattern == "dealt" and n >= 63:
        assert set(want["k_of"].tolist()) == {1, 2, 3} or set(want["k_of"].tolist()) == {2, 3}
    elif pattern == "cloud" and n >= 255:
        assert 0.4 * n <= removed <= 0.8 * n, removed
    elif pattern == "special" and n >= 255:
        assert (~ref.cells(means, ref.h_of(h)[0])[0]).sum() >= 5 and removed > 0
    got = _run(means, colors, stamps, h)
    _check(got, want, n)
    again = _run(means, colors, stamps, h)
    for name in ("first", "second", "counters"):
        assert again[name] == got[name]
    assert np.array_equal(again["kept"], got["kept"])
    for name in ("ids", "means", "colors", "stamps"):
        assert np.array_equal(_u32(again[name]), _u32(got[name])), name


def test_argument_refusals():
    lib, ptr = _lib.load_library(), _lib.ptr
    n = 100
    full = lib.gsl_map_merge_ws_bytes(n)
    m = torch.zeros(n, 3, device=DEV)
    s = torch.full((n,), 5, dtype=torch.int32, device=DEV)
    counters = torch.full((4,), -5, dtype=torch.int32, device=DEV)
    ws = torch.zeros(full, dtype=torch.uint8, device=DEV)
    good = dict(means=ptr(m), colors=ptr(m), stamps=ptr(s), n_rows=n, inv_h=4.0, h=0.25, counters=ptr(counters),
                ws=ptr(ws), ws_bytes=full, stream=None)
    for over in (dict(means=None), dict(stamps=None), dict(ws=None), dict(n_rows=0), dict(n_rows=2 ** 31), dict(h=0.0),
                 dict(h=float("nan")), dict(inv_h=float("inf")), dict(inv_h=-1.0)):
        assert lib.gsl_map_merge_select(*dict(good, **over).values()) == BAD_ARG, over
    assert lib.gsl_map_merge_select(*dict(good, ws_bytes=full - 1).values()) == WORKSPACE
    good = dict(ids=ptr(s), counters=ptr(counters), n_rows=n, out_means=ptr(m), out_colors=ptr(m), out_stamps=ptr(s),
                ws=ptr(ws), ws_bytes=full, stream=None)
    for over in (dict(ids=None), dict(counters=None), dict(out_means=None), dict(out_stamps=None), dict(ws=None),
                 dict(n_rows=0), dict(n_rows=2 ** 31)):
        assert lib.gsl_map_merge_apply(*dict(good, **over).values()) == BAD_ARG, over
    assert lib.gsl_map_merge_apply(*dict(good, ws_bytes=full - 1).values()) == WORKSPACE
    torch.cuda.synchronize()
    assert counters.tolist() == [-5] * 4 and not bool(ws.any()) and not bool(m.any())  # nothing was launched


# ---- GaussianMap ----------------------------------------------------------------------------------------------------
def _filled(cap, means, colors, stamps, **cfg):
    n = len(means)
    m = GaussianMap(W, H, MapConfig(capacity=cap, **cfg), DEV)
    m.means[:n], m.colors[:n], m.n_live = torch.from_numpy(means).to(DEV), torch.from_numpy(colors).to(DEV), n
    m.stamps[:n] = torch.from_numpy(stamps).to(DEV)
    return m


def test_a_map_merges_what_the_mirror_says():
    n, cap = 30000, 40000
    means, colors, stamps, h = _case(n, "cloud")
    want = ref.merge(means, colors, stamps, h)
    k = len(want["ids"])
    assert 0.4 * n <= n - k <= 0.8 * n
    m = _filled(cap, means, colors, stamps, merge_voxel=h)
    mptr, m._view_rows = m.means.data_ptr(), n
    assert m.merge() == (n - k, k) and m.n_live == k and m._view_rows == -1
    assert m.means.data_ptr() != mptr and m._free["means"].data_ptr() == mptr  # a swap
    assert np.array_equal(m.survivors.cpu().numpy(), want["ids"])
    assert np.array_equal(_u32(m.points.cpu().numpy()), _u32(want["means"]))
    assert np.array_equal(_u32(m.point_colors.cpu().numpy()), _u32(want["colors"]))
    assert np.array_equal(m.stamps[:k].cpu().numpy(), want["stamps"])
    # fused rows stay in their voxel: a second merge finds nothing, and then nothing changes, not even a bit --
    # the very same tensors, the spare ones included
    assert ref.occupancy(want["means"], h) == 1
    tensors = (m.means, m.colors, m.stamps, m._free["means"], m._free["colors"], m._free["stamps"])
    before = [(t.data_ptr(), t.clone()) for t in tensors]
    assert m.merge() == (0, k) and m.n_live == k
    after = (m.means, m.colors, m.stamps, m._free["means"], m._free["colors"], m._free["stamps"])
    for (p, old), new in zip(before[:3], after[:3]):
        assert new.data_ptr() == p and torch.equal(new.view(torch.int32), old.view(torch.int32))
    assert [t.data_ptr() for t in after[3:]] == [p for p, _ in before[3:]]
    assert np.array_equal(m.survivors.cpu().numpy(), np.arange(k))
    with pytest.raises(RuntimeError, match="merge_voxel"):
        _filled(cap, means, colors, stamps).merge()
