"""GPU: gsl_map_place_describe and gsl_map_place_match (csrc/map_place.hip) against the numpy mirror
tests/map_place_ref.py, bit for bit, and GaussianMap.describe / add_keyframe / match_place on the device.

The descriptor: images of 16x12 (one pixel per cell), 33x17 (cells of 2 or 3 columns by 1 or 2 lines), 160x120 (cells of
10x10: less than one wave has work in the second trip), 333x171 (uneven cells of up to 21x15 = 315 pixels: two trips of a
256-thread workgroup) and 640x480 (40x40: seven trips); each with all pixels valid, with a tenth of the pixels NaN / inf
/ 0 / negative, and with whole cells empty as well (plus one cell exactly half valid and one a pixel short of it).  The
depths are uniform in 0.25 .. 8 m with a few above the 63 m clamp.  desc is handed over filled with 0x7f bytes and has a
guard region behind it.  One image of 4096x3072 at 100 m everywhere holds the largest cell the entry point takes, 65 536
pixels of 64 512: the sum that just fits 32 bits.

The match: 1, 2, 255 and 256 keyframes of random descriptors (a fifth of the entries invalid), one of them all invalid,
one equal to the query.  out has a guard region behind it.

Every refusal of tests/test_map_place_cpu.py is repeated with device pointers: nothing is written."""
import numpy as np
import pytest
import torch

from gsplatloc_amd import _lib
from gsplatloc_amd.mapping import GaussianMap, MapConfig
from gsplatloc_amd.synthetic import replica_intrinsics, room_depth
from tests import map_place_ref as ref
from tests import test_map_score_cpu as score_cpu
from tests.test_abi import prototypes
from tests.test_map_place_cpu import DESCRIBE, GOOD, MATCH, REFUSED

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
FILL = 0x7F7F7F7F
GUARD = 64
SIZES = [(16, 12), (33, 17), (160, 120), (333, 171), (640, 480)]
KINDS = ["valid", "tenth_bad", "empty_cells"]


def _image(w, h, kind, seed):
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.25, 8.0, size=(h, w)).astype(F32)
    d[rng.random((h, w)) < 0.01] = F32(70.0)  # above the clamp
    if kind != "valid":
        bad = rng.random((h, w)) < 0.1
        d[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.5], F32), size=int(bad.sum()))
    if kind == "empty_cells":
        ci = (np.arange(w) * 16) // w
        cj = (np.arange(h) * 12) // h
        cell = cj[:, None] * 16 + ci[None, :]
        for c in rng.choice(192, size=40, replace=False):
            d[cell == c] = 0.0
        for c, short in ((5, 0), (100, 1)):  # exactly half of the cell's pixels valid; one short of half
            at = np.argwhere(cell == c)
            n_valid = (len(at) + 1) // 2 - short
            for k, (v, u) in enumerate(at):
                d[v, u] = F32(2.0) if k < n_valid else F32(0.0)
    return d


def _describe(depth):
    lib = _lib.load_library()
    h, w = depth.shape
    dev = torch.from_numpy(depth).to(DEV)
    out = torch.full((192 + GUARD,), FILL, dtype=torch.int32, device=DEV)
    _lib.check(lib.gsl_map_place_describe(_lib.ptr(dev), w, h, _lib.ptr(out), _lib.current_stream()), DESCRIBE)
    out = out.cpu().numpy()
    assert (out[192:] == FILL).all()
    return out[:192]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_descriptor_equals_the_mirror(size, kind):
    w, h = size
    depth = _image(w, h, kind, seed=w + 7 * KINDS.index(kind))
    want = ref.describe(depth)
    got = _describe(depth)
    assert got.dtype == np.int32 and np.array_equal(got, want), np.argwhere(got != want)[:5]
    if kind == "valid":
        assert (want >= 0).all()
    if kind == "empty_cells":
        assert (want == -1).sum() >= 40 and want[5] == 2048 and want[100] == -1


def test_descriptor_of_the_largest_cell_the_entry_point_takes():
    """4096 x 3072: every cell is 256 x 256 = 65 536 pixels; at 100 m every pixel clamps to 64 512 and the cell's sum is
    65 536 x 64 512 = 4 227 858 432, below 2^32.  One column more is refused."""
    lib = _lib.load_library()
    depth = torch.full((3072, 4096), 100.0, device=DEV)
    out = torch.full((192,), FILL, dtype=torch.int32, device=DEV)
    _lib.check(lib.gsl_map_place_describe(_lib.ptr(depth), 4096, 3072, _lib.ptr(out), _lib.current_stream()), DESCRIBE)
    assert out.cpu().tolist() == [64512] * 192
    depth[:, ::2] = 0.0  # half of every cell: still valid, the same mean
    depth[5, 1] = 0.0  # cell (0, 0) one short of half
    _lib.check(lib.gsl_map_place_describe(_lib.ptr(depth), 4096, 3072, _lib.ptr(out), _lib.current_stream()), DESCRIBE)
    assert out.cpu().tolist() == [-1] + [64512] * 191
    out.fill_(FILL)
    assert lib.gsl_map_place_describe(_lib.ptr(depth), 4097, 3072, _lib.ptr(out), _lib.current_stream()) == score_cpu.BAD_ARG
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == FILL).all()


def _descriptors(n, seed):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, ref.Q_MAX + 1, size=(n, 192)).astype(np.int32)
    t[rng.random((n, 192)) < 0.2] = -1
    return t


@pytest.mark.parametrize("n", [1, 2, 255, 256])
def test_match_equals_the_mirror(n):
    lib = _lib.load_library()
    table = _descriptors(n, seed=n)
    query = _descriptors(1, seed=1000 + n)[0]
    table[(n - 1) // 2] = -1  # an all-invalid descriptor
    table[n - 1] = query  # the query itself
    out = torch.full((n * 15 * 2 + GUARD,), FILL, dtype=torch.int32, device=DEV)
    q_dev, t_dev = torch.from_numpy(query).to(DEV), torch.from_numpy(table).to(DEV)
    _lib.check(lib.gsl_map_place_match(_lib.ptr(q_dev), _lib.ptr(t_dev), n, _lib.ptr(out), _lib.current_stream()), MATCH)
    got = out.cpu().numpy()
    assert (got[n * 30:] == FILL).all()
    got = got[:n * 30].reshape(n, 15, 2).astype(np.int64)
    want = ref.match(query, table)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    # the query against itself: its (0, 0) shift has sum 0 and all of its valid cells in common
    assert got[n - 1, 7].tolist() == [int((query >= 0).sum()), 0]
    if n > 1:
        assert (got[(n - 1) // 2] == 0).all()  # nothing in common with the all-invalid descriptor


@pytest.mark.parametrize("fn", [DESCRIBE, MATCH])
def test_refusals_write_nothing_on_the_device(fn, repo_root, monkeypatch):
    monkeypatch.setattr(score_cpu, "FN", fn)
    lib = _lib.load_library()
    params = prototypes(repo_root)[fn][1]
    buf = torch.full((1 << 16,), FILL, dtype=torch.int32, device=DEV)
    pointers = {n: buf.data_ptr() for t, n in params if "*" in t}
    for what, over in REFUSED[fn]:
        assert score_cpu.call_with(lib, params, dict(GOOD[fn], **over), pointers) == score_cpu.BAD_ARG, (fn, what)
    torch.cuda.synchronize()
    assert bool((buf == FILL).all())


def test_gaussian_map_keyframes_on_the_device():
    """describe, add_keyframe and match_place with the real launches: the table's rows, the ring, and the ranking of
    the mirror on host copies."""
    w, h = 160, 120
    K = replica_intrinsics(w, h)
    m = GaussianMap(w, h, MapConfig(reloc=True, keyframes=True, keyframe_max=3, keyframe_rot_deg=20.0))
    poses = []
    for k in range(4):
        c2w = torch.eye(4)
        c, s = np.cos(np.radians(50.0 * k)), np.sin(np.radians(50.0 * k))
        c2w[0, 0], c2w[0, 2], c2w[2, 0], c2w[2, 2] = c, s, -s, c
        c2w[:3, 3] = torch.tensor([0.6, 0.1, 0.8])
        poses.append(c2w)
    depths = [room_depth(w, h, K, p) for p in poses]
    got = m.describe(depths[0])
    assert got.is_cuda and got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), ref.describe(depths[0].numpy()))
    assert [m.add_keyframe(d, p) for d, p in zip(depths[:3], poses[:3])] == [0, 1, 2]
    assert m.add_keyframe(depths[1], poses[1]) is None
    assert m.add_keyframe(depths[3], poses[3]) == 0 and m.n_keyframes == 3  # the ring
    table = np.stack([ref.describe(depths[k].numpy()) for k in (3, 1, 2)])
    assert np.array_equal(m._place["table"].cpu().numpy(), table)
    ranked = m.match_place(depths[2])
    assert ranked == ref.rank(ref.match(ref.describe(depths[2].numpy()), table), 48)
    assert ranked[0] == (2, 0, 0, 0, 192) and len(ranked) == 3
