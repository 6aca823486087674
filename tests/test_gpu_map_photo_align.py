"""GPU: gsl_map_pose_align_photo and gsl_map_pose_align_batch_photo (csrc/map_align.hip, csrc/map_align_batch.hip with
the sums of csrc/map_photo.hip) against the numpy mirror tests/map_photo_ref.py on the textured wall, at 33x17 and at
160x120: the pose, the working copy, the steps, the done word, every history row and the sums left behind, bit for
bit.  A batch of the start and three perturbed starts equals the four single calls; a pose that closes early leaves the
sums of gsl_map_pose_info_photo at its final pose.  All buffers lie inside guard words, the inputs keep their bits."""
import math

import numpy as np
import pytest
import torch

from gsplatloc_amd import _lib
from tests import map_align_ref as align
from tests import map_photo_ref as ref
from tests.test_map_photo_cpu import WALL_BOUND

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
NEAR = 0.01
KEEP, BEYOND, KAPPA = ref.keep_of(0.05), ref.beyond_of(0.05), F32(1e-3)
SCALE, RMAX = 0.2, 0.1
STEPS = 8
PARAMS = (STEPS, 1e-3, 7, math.radians(12.8), 0.32, math.radians(1.5e-4), 3e-5)  # MapConfig's defaults
STATE, ROW, VALUES = 14, 10, 30
FILL = 0x7F7F7F7F7F7F7F7F
GUARD = 8
SIZES = {"33x17": (33, 17, (16.0, 16.0, 16.0, 8.0)), "160x120": (ref.WALL_W, ref.WALL_H, ref.WALL_INTR)}
# the start and three starts a millimetre and a few hundredths of a degree from it
TWISTS = [np.zeros(6), np.array([0.0, 0.0, 6e-4, 1e-3, 0.0, 0.0]), np.array([2e-4, -3e-4, 0.0, 0.0, -1.5e-3, 5e-4]),
          np.array([0.0, 1e-4, -8e-4, -2e-3, 1e-3, 0.0])]


@pytest.fixture(scope="module")
def walls():
    out = {}
    for name, (w, h, intr) in SIZES.items():
        c = ref.wall_case(0.3 if name == "33x17" else 0.0, w, h, intr)
        c["starts"] = np.stack([(ref.twist_pose(xi) @ np.eye(4)).astype(F32) for xi in TWISTS])
        out[name] = c
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class _Device:
    """The wall's arrays on the device, and the entry points on buffers inside guard words."""

    def __init__(self, c):
        self.c = c
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
        self.host = (c["means"], c["colors"], c["depth"], c["image"])
        self.means, self.colors, self.depth, self.image = (t(a) for a in self.host)
        self.h, self.w = c["depth"].shape

    def _common(self):
        return (*(float(a) for a in self.c["intr"]), _lib.ptr(self.depth), self.w, self.h, float(KEEP), float(BEYOND),
                float(KAPPA), NEAR)

    def unchanged(self):
        for dev, was in zip((self.means, self.colors, self.depth, self.image), self.host):
            assert np.array_equal(_bits(dev.cpu().numpy()), _bits(was))

    def align(self, starts, batch):
        """Per pose (P [3,4] float64, work [4,4] float32, steps_taken, done, rows [STEPS,4], xis [STEPS,6], sums [30])."""
        lib, ptr, st = _lib.load_library(), _lib.ptr, _lib.current_stream()
        k = len(starts)
        sizes = [k * VALUES, k * 8, k * STATE, k * STEPS * ROW]  # sums, work, state, history in 8-byte words
        offs, at = [], GUARD
        for s in sizes:
            offs.append(at)
            at += s + GUARD
        buf = torch.full((at,), FILL, dtype=torch.int64, device=DEV)
        base = buf.data_ptr()
        p_sums, p_work, p_state, p_hist = (base + 8 * o for o in offs)
        start = torch.from_numpy(np.ascontiguousarray(starts.reshape(k, 16))).to(DEV)
        tail = (*PARAMS, p_sums, p_work, p_state, p_hist, ptr(self.colors), ptr(self.image), SCALE, RMAX, st)
        n = len(self.c["means"])
        if batch:
            _lib.check(lib.gsl_map_pose_align_batch_photo(ptr(self.means), n, ptr(start), k, *self._common(), *tail),
                       "gsl_map_pose_align_batch_photo")
        else:
            assert k == 1
            _lib.check(lib.gsl_map_pose_align_photo(ptr(self.means), n, ptr(start), *self._common(), *tail),
                       "gsl_map_pose_align_photo")
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        keep = np.ones(at, bool)
        for o, s in zip(offs, sizes):
            keep[o:o + s] = False
        assert (host[keep] == FILL).all()  # the guard words
        assert np.array_equal(_bits(start.cpu().numpy()), _bits(starts.reshape(k, 16)))
        out = []
        for p in range(k):
            state = host[offs[2] + p * STATE:offs[2] + (p + 1) * STATE]
            hist = host[offs[3] + p * STEPS * ROW:offs[3] + (p + 1) * STEPS * ROW].reshape(STEPS, ROW)
            out.append((state[:12].copy().view(np.float64).reshape(3, 4),
                        host[offs[1] + p * 8:offs[1] + (p + 1) * 8].copy().view(F32).reshape(4, 4), int(state[12]),
                        int(state[13]), hist[:, :4].copy(), hist[:, 4:].copy().view(np.float64),
                        host[offs[0] + p * VALUES:offs[0] + (p + 1) * VALUES].copy()))
        return out

    def info(self, work):
        lib, ptr, st = _lib.load_library(), _lib.ptr, _lib.current_stream()
        w_t = torch.from_numpy(np.ascontiguousarray(work.reshape(16))).to(DEV)
        out = torch.zeros(VALUES + 2, dtype=torch.int64, device=DEV)
        _lib.check(lib.gsl_map_pose_info_photo(ptr(self.means), len(self.c["means"]), ptr(w_t), *self._common(),
                                               out.data_ptr(), ptr(self.colors), ptr(self.image), SCALE, RMAX,
                                               out[VALUES:].data_ptr(), st), "gsl_map_pose_info_photo")
        return out.cpu().numpy()[:VALUES]


def _mirror(c, start):
    return ref.pose_align(c["means"], c["colors"], start, c["intr"], c["depth"], c["image"], KEEP, BEYOND, KAPPA, NEAR,
                          SCALE, RMAX, *PARAMS)


def _same(got, want, what, done=True, sums=True):
    P, work, taken, flag, hist, xis, s = got
    wP, wwork, wtaken, wflag, whist, wxis, ws = want
    assert np.array_equal(P.view(np.uint64), wP.view(np.uint64)), what
    assert np.array_equal(_bits(work), _bits(wwork)), what
    assert taken == wtaken and (not done or flag == wflag), (what, taken, wtaken, flag, wflag)
    assert np.array_equal(hist, whist), (what, hist, whist)
    assert np.array_equal(xis.view(np.uint64), wxis.view(np.uint64)), what
    if sums:
        assert np.array_equal(s, ws), what


@pytest.mark.parametrize("name", list(SIZES))
def test_the_single_alignment_against_the_mirror(name, walls):
    c = walls[name]
    dev = _Device(c)
    want = _mirror(c, c["starts"][0])
    assert want[2] >= 2 and want[4][0, 1] > (c["depth"].size // 2)  # it moved, on most of the image
    if name == "160x120":
        assert want[4][-1, 0] == align.CONVERGED and ref.pose_error(want[0], c["truth"])[0] <= WALL_BOUND[0.0][0]
    got = dev.align(c["starts"][:1], batch=False)[0]
    _same(got, want, name)
    again = dev.align(c["starts"][:1], batch=False)[0]
    _same(again, got, name + ", twice")
    dev.unchanged()


@pytest.mark.parametrize("name", list(SIZES))
def test_the_batch_is_the_single_calls_and_the_mirror(name, walls):
    c = walls[name]
    dev = _Device(c)
    batch = dev.align(c["starts"], batch=True)
    wants = ref.pose_align_batch(c["means"], c["colors"], c["starts"], c["intr"], c["depth"], c["image"], KEEP, BEYOND,
                                 KAPPA, NEAR, SCALE, RMAX, *PARAMS)
    closed = 0
    for p, (got, want) in enumerate(zip(batch, wants)):
        _same(got, want, (name, p))
        single = dev.align(c["starts"][p:p + 1], batch=False)[0]
        # the single call's done word has two values and its sums are the last iteration's: the same integers once the
        # pose has stopped moving
        _same(got, single, (name, p, "single"), done=False)
        if got[3] == 2:
            # closed early: the sums are those of the photometric entry point at the final working pose
            closed += 1
            assert got[2] < STEPS or got[4][-1, 0] != align.STEPPED
            assert np.array_equal(got[6], dev.info(got[1])), (name, p)
            want_info, _ = ref.pose_info(c["means"], c["colors"], got[1], c["intr"], c["depth"], c["image"], KEEP, BEYOND,
                                         KAPPA, NEAR, SCALE, RMAX)
            assert np.array_equal(got[6], want_info), (name, p)
    if name == "160x120":
        assert closed == len(TWISTS)  # every start converges on this wall, before the last iteration
    dev.unchanged()


def test_a_loop_constraint_reads_the_prefix_and_its_colours(walls):
    """GaussianMap.loop_constraint(intensity=) against the mirror on the rows of frame 0 alone: a second frame, inserted
    5 cm off with other colours, lies behind the prefix in the map and must take no part -- neither its rows nor its
    colours.  The pose, the status and every history row are the mirror's."""
    import torch

    from gsplatloc_amd.mapping import ALIGN_STATUS, GaussianMap, MapConfig

    c = walls["160x120"]
    w, h = ref.WALL_W, ref.WALL_H
    fx, fy, cx, cy = ref.WALL_INTR
    K = torch.tensor([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
    m = GaussianMap(w, h, MapConfig(origins=True, align=True, photo_scale=SCALE, photo_max_residual=RMAX), DEV)
    d0, rgb0 = ref.wall_frame(np.eye(4))
    assert m.insert_frame(torch.from_numpy(d0), torch.from_numpy(rgb0), K, torch.eye(4), origin=0) == (w * h, w * h)
    off = torch.eye(4)
    off[0, 3], off[2, 3] = 0.03, -0.05
    m.insert_frame(torch.from_numpy(c["depth"]), torch.from_numpy(255.0 - c["rgb"]), K, off, origin=1)
    assert m.n_live > w * h and m.rows_up_to(0) == w * h
    image = m.intensity(torch.from_numpy(c["rgb"]))
    assert np.array_equal(_bits(image.cpu().numpy()), _bits(c["image"]))
    got = m.loop_constraint(torch.from_numpy(c["depth"]), K, torch.eye(4), 0, NEAR, intensity=image)
    means, colors = m.points[:w * h].cpu().numpy(), m.point_colors[:w * h].cpu().numpy()
    P, _, taken, _, hist, xis, _ = ref.pose_align(means, colors, np.eye(4, dtype=F32), c["intr"], c["depth"], c["image"],
                                                  KEEP, BEYOND, KAPPA, NEAR, SCALE, RMAX, *PARAMS)
    al = got.alignment
    assert got.rows == w * h and al.steps == taken and al.status == ALIGN_STATUS[hist[-1, 0]] == "CONVERGED"
    assert np.array_equal(al.w2c64[:3].view(np.uint64), P.view(np.uint64))
    assert [(ALIGN_STATUS.index(s), u, t) for s, u, t, _, _ in al.history] == [tuple(r[:3]) for r in hist.tolist()]
    assert all(np.array_equal(x.view(np.uint64), want.view(np.uint64)) for (_, _, _, _, x), want in zip(al.history, xis))
    assert ref.pose_error(P, c["truth"])[0] <= WALL_BOUND[0.0][0]
    # every row of the map, the second frame's included, gives another pose: the prefix is what made the difference
    everything = m.align_pose(torch.from_numpy(c["depth"]), K, torch.eye(4), NEAR, intensity=image)
    assert not np.array_equal(everything.w2c64, al.w2c64)
