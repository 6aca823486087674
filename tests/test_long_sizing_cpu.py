"""Host sizing of the long-list workspace (no GPU needed): RenderContext._alloc_long, grow_long and grow_bins keep their
own policies -- what counts as near-long, the three extra copies of the longest list, max() with the old values, the
factor 4 -- and share the step that turns (long_min, segments, longest list) into the state.  The expected tuples
(long_min, max_seg, long_passes, long_ws_bytes) were recorded from the code before that step was shared."""
import pytest
import torch

PILE = [100] * 11 + [3000]
SHORT = [100] * 11 + [1400]
FRAME = [2000] * 6 + [9000, 7000, 23000, 0, 0, 5]
BUSY = [700] * 11 + [2600]
OFF = (0, 0, 0, 0)

# (tile sizes, headroom) -> state after _alloc_long, after a following grow_long(10), after a following grow_long(300)
ALLOC = [
    (PILE, 1.3, (2048, 152, 4, 1094064), (2048, 152, 4, 1094064), (2048, 458, 7, 3296040)),
    (SHORT, 1.3, OFF, (2048, 23, 2, 165780), (2048, 458, 7, 3296040)),
    (FRAME, 1.3, (20402, 1088, 7, 7829520), (20402, 1088, 7, 7829520), (20402, 1088, 7, 7829520)),
    (FRAME, 2.0, (20402, 1448, 7, 10420080), (20402, 1448, 7, 10420080), (20402, 1448, 7, 10420080)),
    ([0] * 12, 1.3, OFF, (2048, 23, 2, 165780), (2048, 458, 7, 3296040)),
    (BUSY, 1.3, (3433, 132, 3, 950144), (3433, 132, 3, 950144), (3433, 458, 7, 3296040)),
]
# (mean list of the calibration, longest list seen) -> state after grow_bins, bin_cap
BINS = [
    (0.0, 1000, OFF, 1564),
    (0.0, 1600, (2048, 84, 3, 604736), 2464),
    (0.0, 23000, (2048, 1088, 7, 7829520), 34564),
    (700.0, 2000, OFF, 3064),
    (700.0, 2200, (2800, 112, 3, 806224), 3364),
    (700.0, 9000, (2800, 432, 5, 3108944), 13564),
]


def _context():
    import gsplatloc_amd.context as CX

    return CX.RenderContext(500, 64, 48, "RGB+ED", sh_degree=1, K_sh=4, device="cpu")


def _state(ctx):
    assert (ctx.long_ws is None) == (ctx.long_ws_bytes == 0)
    assert ctx.long_ws is None or (ctx.long_ws.numel() == ctx.long_ws_bytes and not ctx.long_ws.any())
    return ctx.long_min, ctx.max_seg, ctx.long_passes, ctx.long_ws_bytes


@pytest.mark.parametrize("sizes,headroom,after_alloc,after_grow_10,after_grow_300", ALLOC)
def test_alloc_long_and_grow_long(sizes, headroom, after_alloc, after_grow_10, after_grow_300):
    for needed, expected in ((10, after_grow_10), (300, after_grow_300)):
        ctx = _context()
        ctx._alloc_long(torch.tensor(sizes, dtype=torch.int32), headroom)
        assert _state(ctx) == after_alloc
        ctx.grow_long(needed)
        assert _state(ctx) == expected


def test_grow_long_without_a_calibrated_workspace():
    ctx = _context()
    ctx.grow_long(40)
    assert _state(ctx) == (2048, 68, 4, 489600)


@pytest.mark.parametrize("mean_list,longest,expected,bin_cap", BINS)
def test_grow_bins(mean_list, longest, expected, bin_cap):
    ctx = _context()
    ctx._mean_list = mean_list
    ctx.grow_bins(longest)
    assert _state(ctx) == expected and ctx.bin_cap == bin_cap


def test_grow_bins_leaves_a_long_list_mode_that_is_already_on():
    ctx = _context()
    ctx._alloc_long(torch.tensor(PILE, dtype=torch.int32), 1.3)
    ws = ctx.long_ws
    ctx.grow_bins(9000)
    assert _state(ctx) == (2048, 152, 4, 1094064) and ctx.long_ws is ws and ctx.bin_cap == 13564
