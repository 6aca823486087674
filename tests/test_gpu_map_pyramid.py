"""GPU: gsl_map_pyramid (csrc/map_pyramid.hip) against the numpy mirror tests/map_pyramid_ref.py, every level of both
images bit for bit (== on the uint32 view), and GaussianMap.pyramid.

The sizes: 160 x 120 with 3 levels (the wall's frame: 5 x 4 tiles, the last row of tiles partly filled); 37 x 29 with 2,
odd at every level; 70 x 45 with 3, no multiple of the tile, so edge tiles that are partly filled at every level;
33 x 36 with 2, whose column 32 falls into a second tile and is dropped; 64 x 64 with 4, four full tiles down to the 2 x
2 block a tile leaves at level 4.  The images are a random slanted surface with a step through it (so that blocks
straddle it), pixels of 0, a negative depth, +inf and NaN scattered over it, and an intensity with a NaN, an inf and
values outside 0 .. 1.

The hand-made frames: every position of the 2 x 2 block in turn holding 0, a negative depth, +inf and NaN; a depth step
whose ratio sits on, and one float32 step to either side of, 1 - rho_p.

Both outputs are handed over inside guard words; the inputs are compared bit for bit after the call."""
import numpy as np
import pytest
import torch

from gsplatloc_amd import _lib
from gsplatloc_amd.mapping import GaussianMap, MapConfig, pyramid_intrinsics
from tests import map_pyramid_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
GUARD = 64  # floats on either side of each output
FILL = -7.0
KEEP = ref.keep_of(0.05)
SIZES = [(160, 120, 3), (37, 29, 2), (70, 45, 3), (33, 36, 2), (64, 64, 4)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _frame(w, h, seed):
    """(depth, intensity) float32 [h,w]: a slanted surface with a step along a slanted line, bad pixels of every kind."""
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    depth = 2.0 + 0.01 * u - 0.004 * v + np.where(u + 0.5 * v > 0.6 * w, 0.5, 0.0) + rng.uniform(0, 2e-3, (h, w))
    depth = depth.astype(F32)
    for k, i in enumerate(rng.permutation(w * h)[:max(4, w * h // 200)]):
        depth.reshape(-1)[i] = [0.0, -1.5, np.inf, np.nan][k % 4]
    image = rng.uniform(0.0, 1.0, (h, w)).astype(F32)
    for k, i in enumerate(rng.permutation(w * h)[:8]):
        image.reshape(-1)[i] = [np.nan, np.inf, -0.25, 9.0][k % 4]
    return depth, image


def _run(depth, image, levels, keep):
    """The entry point on outputs inside guard words: (packed depth levels, packed intensity levels or None)."""
    lib, ptr, st = _lib.load_library(), _lib.ptr, _lib.current_stream()
    h, w = depth.shape
    n = lib.gsl_map_pyramid_floats(w, h, levels)
    assert n == ref.floats(w, h, levels) > 0
    d_t = torch.from_numpy(depth).to(DEV)
    y_t = None if image is None else torch.from_numpy(image).to(DEV)
    buf = torch.full((2, n + 2 * GUARD), FILL, device=DEV)
    _lib.check(lib.gsl_map_pyramid(ptr(d_t), ptr(y_t), w, h, levels, float(keep), buf[0, GUARD:].data_ptr(),
                                   None if image is None else buf[1, GUARD:].data_ptr(), st), "gsl_map_pyramid")
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:, :GUARD] == FILL).all() and (host[:, GUARD + n:] == FILL).all()  # the guards on both sides of both
    if image is None:
        assert (host[1] == FILL).all()
    assert np.array_equal(_bits(d_t.cpu().numpy()), _bits(depth))  # the inputs are only read
    if image is not None:
        assert np.array_equal(_bits(y_t.cpu().numpy()), _bits(image))
    return host[0, GUARD:GUARD + n].copy(), None if image is None else host[1, GUARD:GUARD + n].copy()


def _check(depth, image, levels, keep=KEEP):
    got_d, got_y = _run(depth, image, levels, keep)
    depths, images, _ = ref.pyramid(depth, levels, keep, image)
    assert np.array_equal(_bits(got_d), _bits(ref.packed(depths)))
    if image is not None:
        assert np.array_equal(_bits(got_y), _bits(ref.packed(images)))
    return depths, images


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}-L{s[2]}")
def test_every_level_against_the_mirror(size):
    w, h, levels = size
    depth, image = _frame(w, h, 100 * w + h)
    depths, images = _check(depth, image, levels)
    assert [d.shape for d in depths[1:]] == [(hh, ww) for ww, hh in ref.sizes(w, h, levels)]
    # the case is one: valid and refused blocks, and pixels refused only because of the step, at level 1
    assert 0 < (depths[1] > 0).mean() < 1 and (depths[-1] > 0).any()
    assert np.isnan(images[1]).any() and (images[1][np.isfinite(images[1])] > 1).any()  # a NaN and a value > 1 survive
    # depth only: the same depths, the intensity output untouched
    _check(depth, None, levels)


def test_every_bad_value_at_every_position_of_the_block():
    """A 16 x 16 frame of depth 2 (8 x 8 blocks, two levels): block k = 4 * value + position holds one bad value; its
    level-1 pixel is 0, and so is the level-2 pixel above it; every other block gives 2 up to rounding."""
    depth = np.full((16, 16), 2.0, F32)
    bad = [0.0, -1.0, np.inf, np.nan]
    for k in range(16):
        i, j = 2 * (k % 8), 2 * (2 * (k // 8))  # blocks of rows 0 and 2 (in blocks): level-1 rows 0 and 2
        depth[j + (k % 4) // 2, i + (k % 4) % 2] = bad[k // 4]
    image = np.linspace(0.0, 1.0, 256, dtype=F32).reshape(16, 16)
    depths, _ = _check(depth, image, 2)
    assert (depths[1][0] == 0).all() and (depths[1][2] == 0).all() and (depths[1][[1, 3, 4, 5, 6, 7]] == 2.0).all()
    assert (depths[2][[0, 1]] == 0).all() and (depths[2][2:] == 2.0).all()


def test_a_step_at_the_bound():
    """max * keep <= min with min one float32 step to either side of the rounded product, in each position of the
    block."""
    keep = ref.keep_of(0.0625)  # 0.9375: products of it are exact for short mantissas
    hi = F32(4.0)
    at = hi * keep
    below, above = np.nextafter(at, F32(0)), np.nextafter(at, F32(np.inf))
    depth = np.full((8, 24), hi, F32)
    for pos in range(4):
        for k, lo in enumerate((below, at, above)):
            depth[2 * pos + pos // 2, 8 * k + 2 * pos + pos % 2] = lo
    depths, _ = _check(depth, None, 1, keep)
    for pos in range(4):
        assert depths[1][pos, pos] == 0 and depths[1][pos, 4 + pos] > 0 and depths[1][pos, 8 + pos] > 0


def test_the_host_layer_gives_views_of_the_same_levels():
    w, h, levels = 70, 45, 3
    depth, image = _frame(w, h, 7)
    m = GaussianMap(w, h, MapConfig(align=True, pyramid_rho=0.05), DEV)
    K = torch.tensor([[61.0, 0.0, 34.25], [0.0, 59.0, 22.0], [0.0, 0.0, 1.0]])
    p = m.pyramid(torch.from_numpy(depth), levels, intensity=torch.from_numpy(image), K=K)
    depths, images, intrs = ref.pyramid(depth, levels, KEEP, image, (61.0, 59.0, 34.25, 22.0))
    assert p.levels == levels and p.keep == float(KEEP) and p.sizes == [(w, h)] + ref.sizes(w, h, levels)
    for l in range(levels + 1):
        assert np.array_equal(_bits(p.depths[l].cpu().numpy()), _bits(depths[l]))
        assert np.array_equal(_bits(p.intensities[l].cpu().numpy()), _bits(images[l]))
        assert p.intrs[l] == tuple(float(a) for a in intrs[l])
    assert p.intrs == pyramid_intrinsics((61.0, 59.0, 34.25, 22.0), levels)
    only = m.pyramid(torch.from_numpy(depth), 2, rho=0.1)
    assert only.intensities is None and only.intrs is None and only.keep == float(ref.keep_of(0.1))
    assert np.array_equal(_bits(only.depths[2].cpu().numpy()), _bits(ref.pyramid(depth, 2, ref.keep_of(0.1))[0][2]))


def test_refusals_with_device_pointers_write_nothing():
    from tests.test_map_pyramid_cpu import BAD_ARG, REFUSED

    lib = _lib.load_library()
    buf = torch.full((4, 4096), FILL, device=DEV)
    good = dict(depth=buf[0].data_ptr(), intensity=buf[1].data_ptr(), width=64, height=48, levels=2, keep=0.95,
                depth_out=buf[2].data_ptr(), intensity_out=buf[3].data_ptr())
    for what, over in REFUSED:
        a = dict(good, **over)
        assert lib.gsl_map_pyramid(a["depth"], a["intensity"], a["width"], a["height"], a["levels"], a["keep"],
                                   a["depth_out"], a["intensity_out"], _lib.current_stream()) == BAD_ARG, what
    torch.cuda.synchronize()
    assert bool((buf == FILL).all())
