"""gsl_tile_sort, every kernel of it, against a plain sort.

The per-tile depth sort decides which Gaussian composites in front of which; no tolerance hides an error there.  It
has three kernels -- k_tile_sort<4> / <5> (one tile per wave, up to 16 / 32 keys per lane in registers) and
k_tile_sort_wg (one tile per workgroup) -- and inside each a block-wise LDS sort for lists too long for the registers
(bitonic_sort_long).  Every case below runs under each kernel, forced through GSL_DEV_TILE_SORT, and the launch counters
(gsl_dev_tile_sort_launches) show that the forced kernel ran.

The keys are built here: (float32 depth bits << 32) | Gaussian id, at tile offsets chosen here.  Expected: a stable CPU
sort of each tile's span (int64 order: every depth here has its sign bit clear, so it is the unsigned order), the
span cut at `capacity` ("positions >= capacity are dropped", include/gsloc_hip.h).  flatten_ids and isect_ids are
compared bit for bit; every position the call must not write -- tiles outside the strip, positions at or beyond
capacity -- must come back untouched, in the outputs and in the key array."""
import pytest
import torch

from gsplatloc_amd._lib import check, current_stream, load_library, ptr
from tests.sort_variants import assert_tile_sort_ran, force_tile_sort, forced_tile_sort

pytestmark = pytest.mark.gpu
DEV = "cuda"
KERNELS = ["wave16", "wave32", "wg"]
CAM_ENC = 3 << (32 + 12)  # camera 3 of a 12-bit tile id space: must be OR-ed into every isect_id
FILL_ID, FILL_ISECT = -7, -0x5A5A5A5A5A5A5A5


def _depth_bits(n, gen, ties=7):
    """n float32 depths (as their int32 bits) spread over many binades (1e-30 .. 1e30), every `ties`-th one equal."""
    e = torch.rand(n, generator=gen, dtype=torch.float64) * 60 - 30
    d = (10.0 ** e).float()
    if ties and n > ties:
        d[::ties] = d[ties // 2]
    return d.view(torch.int32).long()


def _keys(bits, ids):
    return (bits << 32) | ids


def _tile(n, gen, id_base=0, ties=7):
    """Keys of one tile list: n distinct Gaussian ids in random order, depths from _depth_bits."""
    ids = id_base + torch.randperm(max(n, 1), generator=gen)[:n].long() * 3
    return _keys(_depth_bits(n, gen, ties), ids)


def _expected(keys, offs, tile_begin, n_strip, capacity, cam_enc):
    """Plain reference: the CPU stable sort of every strip tile's span cut at capacity; everything else untouched."""
    fl = torch.full((keys.numel(),), FILL_ID, dtype=torch.int32)
    ii = torch.full((keys.numel(),), FILL_ISECT, dtype=torch.int64)
    sk = keys.clone()
    for t in range(tile_begin, tile_begin + n_strip):
        s, e = int(offs[t]), min(int(offs[t + 1]), capacity)
        if e <= s:
            continue
        srt = torch.sort(keys[s:e], stable=True).values
        sk[s:e] = srt
        fl[s:e] = (srt & 0xFFFFFFFF).to(torch.int32)
        ii[s:e] = cam_enc | (t << 32) | (srt >> 32)
    return fl, ii, sk


def _run(kernel, monkeypatch, lists, tile_begin=0, n_strip=None, capacity=None, isect=True, cam_enc=CAM_ENC):
    """One gsl_tile_sort call under `kernel` over tiles whose unsorted key lists are `lists` (int64 tensors); the strip
    is tiles [tile_begin, tile_begin + n_strip).  Compared with _expected."""
    lib = load_library()
    n_strip = len(lists) - tile_begin if n_strip is None else n_strip
    sizes = torch.tensor([0] + [int(x.numel()) for x in lists], dtype=torch.int64)
    offs = torch.cumsum(sizes, 0).to(torch.int32)
    keys = torch.cat(lists) if lists else torch.zeros(0, dtype=torch.int64)
    total = keys.numel()
    capacity = total if capacity is None else capacity
    k_d, offs_d = keys.to(DEV), offs.to(DEV)
    fl_d = torch.full((total,), FILL_ID, dtype=torch.int32, device=DEV)
    ii_d = torch.full((total,), FILL_ISECT, dtype=torch.int64, device=DEV) if isect else None
    with forced_tile_sort(monkeypatch, kernel):
        check(lib.gsl_tile_sort(ptr(offs_d), tile_begin, n_strip, capacity, ptr(k_d), ptr(fl_d), ptr(ii_d),
                                cam_enc, current_stream()), "gsl_tile_sort")
        torch.cuda.synchronize()
    fl_w, ii_w, sk_w = _expected(keys, offs.long(), tile_begin, n_strip, capacity, cam_enc)
    fl_g, k_g = fl_d.cpu(), k_d.cpu()
    assert torch.equal(fl_g, fl_w), _first_diff(fl_g, fl_w, offs)
    if isect:
        assert torch.equal(ii_d.cpu(), ii_w), _first_diff(ii_d.cpu(), ii_w, offs)
    # the key array is scratch inside a strip tile's cut span (the long-list sort works there in place); everywhere
    # else it must be as given, and inside those spans it must still hold the same keys
    inside = torch.zeros(total, dtype=torch.bool)
    for t in range(tile_begin, tile_begin + n_strip):
        inside[int(offs[t]):max(int(offs[t]), min(int(offs[t + 1]), capacity))] = True
    assert torch.equal(k_g[~inside], keys[~inside]), "keys outside the sorted spans were written"
    for t in range(tile_begin, tile_begin + n_strip):
        s, e = int(offs[t]), min(int(offs[t + 1]), capacity)
        if e > s:
            assert torch.equal(torch.sort(k_g[s:e]).values, sk_w[s:e]), f"tile {t}: the key scratch lost keys"


def _first_diff(a, b, offs):
    bad = (a != b).nonzero()
    if not bad.numel():
        return "equal"
    i = int(bad[0])
    t = int(torch.searchsorted(offs.long(), torch.tensor([i]), right=True)[0]) - 1
    return f"{int(bad.numel())} positions differ, first {i} (tile {t}, span {int(offs[t])}..{int(offs[t + 1])})"


LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097,
           8193, 20011]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n", LENGTHS)
def test_one_list_at_every_size_class_boundary(n, kernel, monkeypatch):
    """One tile list of every length around the size classes: 4 / 8 / 16 / 32 keys per lane (wave kernels), the LDS
    sorts of the workgroup kernel, and beyond them the block-wise long-list sort with whole and partial blocks.  The
    strip starts at tile 1: tile 0 (37 keys) is outside it and must stay untouched.  With and without isect_ids (the
    wave sort writes flatten_ids through LDS when neither isect_ids nor the sorted keys are wanted)."""
    gen = torch.Generator().manual_seed(1000 + n)
    lists = [_tile(37, gen), _tile(n, gen, id_base=5)]
    for isect in (True, False):
        _run(kernel, monkeypatch, lists, tile_begin=1, isect=isect)


MIXED = {
    "long_short_mid_empty": [3000, 5, 1500, 0],
    "three_empty_then_long": [0, 0, 0, 9000],
    "around_1024_and_2048": [1025, 2049, 1024, 2048],
    "long_neighbours_across_workgroups": [1, 2, 3, 5000, 6000, 2, 1, 0, 4097, 4100, 3, 700],
    "every_class_in_one_launch": [2049, 1, 300, 1025, 64, 4096, 513, 0, 8193, 257, 2048, 65, 1024],
}


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("case", sorted(MIXED))
def test_mixed_neighbours_in_one_workgroup(case, kernel, monkeypatch):
    """The wave kernels put 4 tiles in one 256-thread workgroup: short lists sorted by single waves share the LDS block
    with the sequential long-list loop of the same workgroup, and long lists of neighbouring workgroups are sorted at
    the same time.  Any write outside a tile's [s, e) shows up in a neighbour."""
    gen = torch.Generator().manual_seed(100 + sorted(MIXED).index(case))
    lists = [_tile(n, gen, id_base=i) for i, n in enumerate(MIXED[case])]
    for isect in (True, False):
        _run(kernel, monkeypatch, lists, isect=isect)


@pytest.mark.parametrize("kernel", KERNELS)
def test_launch_geometry_strip_partial_group_and_capacity(kernel, monkeypatch):
    """A strip that starts at tile 3 and covers 7 tiles (not a multiple of 4: the last workgroup of a wave kernel has
    idle waves), the tiles outside it untouched; then `capacity` cutting a tile's span: that tile's first entries
    up to capacity are sorted among themselves, every later position is left alone (a short list, a wave-sorted one
    and a long one each cut)."""
    gen = torch.Generator().manual_seed(77)
    sizes = [40, 0, 900, 130, 1, 2000, 77, 513, 5000, 64, 300]
    lists = [_tile(n, gen, id_base=i) for i, n in enumerate(sizes)]
    for isect in (True, False):
        _run(kernel, monkeypatch, lists, tile_begin=3, n_strip=7, isect=isect)
    starts = [0]
    for n in sizes:
        starts.append(starts[-1] + n)
    for t, keep in ((3, 71), (5, 1500), (8, 3333), (7, 0)):
        _run(kernel, monkeypatch, lists, tile_begin=0, n_strip=len(sizes), capacity=starts[t] + keep)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n", [100, 700, 1500, 3000])
def test_key_content_ties_extremes_zero_and_large_ids(n, kernel, monkeypatch):
    """Keys at the edges of what the sorts may see: one depth for the whole list with ids out of order (the order comes
    from the id alone); depths at the extremes of the float range -- the smallest subnormal and normal, the largest
    finite float, +inf -- and +0.0; ids just below 2^26.  Lengths through the wave sorts and the long-list sort."""
    gen = torch.Generator().manual_seed(n)
    ids = (1 << 26) - 1 - torch.randperm(n, generator=gen).long() * 5
    tie = _keys(torch.full((n,), int(torch.tensor(2.5).view(torch.int32)), dtype=torch.int64), ids)
    special = torch.tensor([0x00000000, 0x00000001, 0x00800000, 0x3F800000, 0x7F7FFFFF, 0x7F800000], dtype=torch.int64)
    bits = special[torch.randint(0, special.numel(), (n,), generator=gen)]
    extreme = _keys(bits, torch.randperm(n, generator=gen).long())
    zero = _keys(torch.zeros(n, dtype=torch.int64), ids)
    for isect in (True, False):
        _run(kernel, monkeypatch, [tie, extreme, zero, _tile(n, gen)], isect=isect)


def test_the_tie_cases_are_ties():
    """Negative control for the reference: in the tie case the expected order comes from the id alone.  A sort by the
    depth alone -- stable, so ties keep their (shuffled) input order -- must disagree with it, and so must a reference
    whose two neighbouring entries are swapped: a kernel that broke ties by input order would fail the comparison."""
    gen = torch.Generator().manual_seed(5)
    n = 700
    ids = torch.randperm(n, generator=gen).long()
    keys = _keys(torch.full((n,), int(torch.tensor(2.5).view(torch.int32)), dtype=torch.int64), ids)
    offs = torch.tensor([0, n])
    fl, _, _ = _expected(keys, offs, 0, 1, n, 0)
    assert torch.equal(fl.long(), torch.arange(n))
    by_depth = torch.sort(keys >> 32, stable=True).indices
    assert not torch.equal((keys[by_depth] & 0xFFFFFFFF).to(torch.int32), fl)
    swapped = fl.clone()
    swapped[[10, 11]] = swapped[[11, 10]]
    assert not torch.equal(swapped, fl)


def test_the_wave32_kernel_itself_sorts_through_the_binned_path(monkeypatch):
    """k_tile_sort<5> behind gsl_fused_bin (RenderContext): offsets from the per-tile counters, keys from the bins,
    lists of 1025..2048 keys -- what only the 32-keys-per-lane network sorts in registers.  The deterministic mode also
    writes the sorted keys (write_sorted_keys), the placed context relabels ids (storage_of).  Expected: the lists of the
    workgroup kernel on the same frame, the sorted keys ascending within every tile with the list's ids as low words,
    and the placed context's lists the plain context's lists relabelled."""
    from gsplatloc_amd.context import RenderContext
    from tests.scenes import small_pose
    from tests.test_gpu_reorder import _wall

    W, H, N = 192, 128, 90000
    means, quats, scales, opac, sh, K = _wall(N, W, H, 1.0, seed=23)
    ins = [t.to(DEV) for t in (means, quats, scales, opac, sh)]
    K = K.to(DEV).contiguous()
    poses = {"wall (all depths tie)": torch.eye(4, device=DEV),
             "moved": torch.linalg.inv(small_pose(0.3, 0.01, dtype=torch.float32)).to(DEV).contiguous()}
    rcs = {"det": RenderContext(N, W, H, "RGB+ED", sh_degree=1, K_sh=4, device=DEV, deterministic=True, reorder=False),
           "placed": RenderContext(N, W, H, "RGB+ED", sh_degree=1, K_sh=4, device=DEV, reorder=True)}
    for rc in rcs.values():
        rc.calibrate(*ins, poses["moved"], K)
        assert rc.bins is not None and (rc.long_min == 0 or rc.long_min > 2048)  # (no list goes to gsl_long_sort)
    assert rcs["placed"].order_ids is not None
    for pose, V in poses.items():
        got = {}
        for kernel in ("wave32", "wg"):
            before = force_tile_sort(monkeypatch, kernel)
            for name, rc in rcs.items():
                rc.forward(*ins, V, K)
                n = rc.check_capacity()
                got[kernel, name] = dict(n=n, offs=rc.offs.clone(), ids=rc.flatten_ids[:n].clone(),
                                         keys=rc.keys[:n].clone() if name == "det" else None)
            torch.cuda.synchronize()
            assert_tile_sort_ran(kernel, before)
        a = got["wave32", "det"]
        sizes = (a["offs"][1:] - a["offs"][:-1]).cpu()
        assert int(((sizes > 1024) & (sizes <= 2048)).sum()) >= 8, (pose, sizes.max())
        for name in rcs:
            x, y = got["wave32", name], got["wg", name]
            assert x["n"] == y["n"] and torch.equal(x["offs"], y["offs"]) and torch.equal(x["ids"], y["ids"]), (pose, name)
        keys, ids, offs = a["keys"].cpu(), a["ids"].cpu(), a["offs"].cpu().long()
        assert torch.equal(keys, got["wg", "det"]["keys"].cpu()), pose
        assert torch.equal((keys & 0xFFFFFFFF).to(torch.int32), ids), pose
        tile_of = torch.repeat_interleave(torch.arange(sizes.numel()), sizes)
        same_tile = tile_of[1:] == tile_of[:-1]
        assert bool((keys[1:] > keys[:-1])[same_tile].all()), f"{pose}: a tile's sorted keys are not ascending"
        placed = got["wave32", "placed"]
        relabelled = rcs["placed"].order_ids.long()[placed["ids"].long()].cpu()
        assert torch.equal(relabelled, ids.long()), f"{pose}: the placed lists are not the plain lists relabelled"


def _bits_as_float(b):
    return torch.tensor([b], dtype=torch.int64).to(torch.int32).view(torch.float32)[0]


BAD_DEPTHS = {"negative": -1.5, "minus_zero": -0.0, "nan": _bits_as_float(0x7FF80000),
              "negative_nan": _bits_as_float(0xFFC00000 - (1 << 32))}


@pytest.mark.parametrize("n", [700, 1500, 3000])
@pytest.mark.parametrize("bad", sorted(BAD_DEPTHS))
def test_isect_tiles_refuses_depths_the_sort_cannot_order(bad, n):
    """gsplat.isect_tiles passes the caller's depths straight into the sort keys.  The sorts compare keys partly as
    doubles and partly as unsigned integers: a visible Gaussian with a negative, -0.0 or NaN depth would get an order
    that depends on the list length (wave sort against long sort, n = 700 / 1500 / 3000 here).  Such a call raises
    ValueError; the same Gaussian with radius 0 (not visible) is accepted, and the lists are the oracle's."""
    import gsplatloc_amd as A
    from oracle import gsplat_oracle as G

    g = torch.Generator().manual_seed(n)
    m2 = (torch.rand(1, n, 2, generator=g) * 14 + 1).float()
    r = torch.full((1, n), 1, dtype=torch.int32)
    d = (torch.rand(1, n, generator=g) * 5 + 0.5).float()
    d[0, n // 2] = BAD_DEPTHS[bad]
    with pytest.raises(ValueError, match="depth"):
        A.isect_tiles(m2.to(DEV), r.to(DEV), d.to(DEV), 16, 2, 2)
    r[0, n // 2] = 0
    _, ids_o, fl_o = G.isect_tiles(m2, r, d, 16, 2, 2)
    _, ids_g, fl_g = A.isect_tiles(m2.to(DEV), r.to(DEV), d.to(DEV), 16, 2, 2)
    assert torch.equal(ids_g.cpu(), ids_o) and torch.equal(fl_g.cpu(), fl_o)
    # (sort=False only emits, in Gaussian order: nothing to order, nothing refused)
    A.isect_tiles(m2.to(DEV), torch.ones_like(r).to(DEV), d.to(DEV), 16, 2, 2, sort=False)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n", [700, 1500, 3000])
def test_isect_tiles_orders_zero_and_infinite_depths_like_the_oracle(n, kernel, monkeypatch):
    """The edges of the accepted depths, +0.0 and +inf (and the largest finite float, the smallest subnormal), on
    visible Gaussians, through every sort kernel at wave and long-list lengths: bit for bit the oracle's lists."""
    import gsplatloc_amd as A
    from oracle import gsplat_oracle as G

    g = torch.Generator().manual_seed(n + 1)
    m2 = (torch.rand(1, n, 2, generator=g) * 14 + 1).float()
    r = torch.full((1, n), 1, dtype=torch.int32)
    d = (torch.rand(1, n, generator=g) * 5 + 0.5).float()
    for i, b in enumerate((0x00000000, 0x7F800000, 0x7F7FFFFF, 0x00000001)):
        d[0, i::9] = _bits_as_float(b)
    _, ids_o, fl_o = G.isect_tiles(m2, r, d, 16, 2, 2)
    with forced_tile_sort(monkeypatch, kernel):
        _, ids_g, fl_g = A.isect_tiles(m2.to(DEV), r.to(DEV), d.to(DEV), 16, 2, 2)
    assert torch.equal(ids_g.cpu(), ids_o) and torch.equal(fl_g.cpu(), fl_o)
