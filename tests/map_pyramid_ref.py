"""numpy mirror of csrc/map_pyramid.hip: the levels of gsl_map_pyramid -- depth by the mean inverse depth of a 2 x 2
block that is valid and does not straddle a step, intensity by the mean of the block -- the intrinsics of a level, and
the coarse-to-fine alignment of GaussianMap.align_pose(levels=) / align_poses(levels=) on top of the mirrors of the two
alignments (tests/map_align_ref.py, tests/map_photo_ref.py), which are imported unchanged: a level is one more call of
theirs with that level's images, size and intrinsics, started at the float32 working pose the level before it left.
float32 with every operation rounded once in the device's order; its own copy of the rule, as the other mirrors have.

And the scene the feature is for: the wall of tests/map_photo_ref.py with a texture whose finest wavelength is about
8.5 pixels, where one level converges from 2 pixels off and not from 4."""
import numpy as np

from tests import map_align_ref as align
from tests import map_photo_ref as photo
from tests.map_align_batch_ref import done_of

F32, F64 = np.float32, np.float64
MAX_LEVELS = 4
MIN_SIDE = 4


def keep_of(rho):
    """1 - rho_p as the host takes it: one float32 subtraction."""
    return F32(1.0) - F32(rho)


def shape_ok(width, height, levels):
    return (0 < width and 0 < height and width * height <= 2 ** 31 - 1 and 1 <= levels <= MAX_LEVELS
            and (width >> levels) >= MIN_SIDE and (height >> levels) >= MIN_SIDE)


def sizes(width, height, levels):
    """[(W_l, H_l)] of levels 1 .. levels."""
    return [(width >> l, height >> l) for l in range(1, levels + 1)]


def floats(width, height, levels):
    """gsl_map_pyramid_floats."""
    return sum(w * h for w, h in sizes(width, height, levels)) if shape_ok(width, height, levels) else 0


def _blocks(x):
    h, w = x.shape[0] // 2, x.shape[1] // 2
    x = x[:2 * h, :2 * w]
    return x[0::2, 0::2], x[0::2, 1::2], x[1::2, 0::2], x[1::2, 1::2]


def depth_level(depth, keep):
    """The next level of a depth image [H,W] float32."""
    a, b, c, e = _blocks(np.asarray(depth, dtype=F32))
    keep, one = F32(keep), F32(1.0)
    with np.errstate(all="ignore"):
        valid = np.ones(a.shape, bool)
        for t in (a, b, c, e):
            valid &= (t > F32(0)) & (t < F32(np.inf))
        # max and min of four values that are all valid: no NaN among them, the order does not matter
        hi, lo = np.maximum(np.maximum(a, b), np.maximum(c, e)), np.minimum(np.minimum(a, b), np.minimum(c, e))
        valid &= hi * keep <= lo
        inv = ((one / a + one / b) + (one / c + one / e)) * F32(0.25)
        out = np.where(valid, one / inv, F32(0))
    assert out.dtype == F32
    return out


def intensity_level(image):
    """The next level of an intensity image [H,W] float32."""
    a, b, c, e = _blocks(np.asarray(image, dtype=F32))
    with np.errstate(all="ignore"):
        out = ((a + b) + (c + e)) * F32(0.25)
    assert out.dtype == F32
    return out


def intr_level(intr):
    """The intrinsics of the next level, float32 values."""
    fx, fy, cx, cy = (F32(a) for a in intr)
    half = F32(0.5)
    return (fx * half, fy * half, (cx - half) * half, (cy - half) * half)


def pyramid(depth, levels, keep, image=None, intr=None):
    """(depths, images or None, intrs or None): lists of levels 0 .. levels, level 0 the inputs as float32; each level
    made from the one before it."""
    depths = [np.asarray(depth, dtype=F32)]
    images = None if image is None else [np.asarray(image, dtype=F32)]
    intrs = None if intr is None else [tuple(F32(a) for a in intr)]
    assert shape_ok(depths[0].shape[1], depths[0].shape[0], levels)
    for _ in range(levels):
        depths.append(depth_level(depths[-1], keep))
        if images is not None:
            images.append(intensity_level(images[-1]))
        if intrs is not None:
            intrs.append(intr_level(intrs[-1]))
    return depths, images, intrs


def packed(levels_list):
    """Levels 1 .. L of a list of images packed one after another, row-major: what the entry point writes."""
    return np.concatenate([x.reshape(-1) for x in levels_list[1:]])


def pose_align(means, colors, w2c, intr, depth, image, keep, beyond, kappa, near, scale, max_residual, max_steps,
               damping, min_used, max_rot, max_trans, eps_rot, eps_trans, levels, level_steps=None, keep_p=None):
    """GaussianMap.align_pose(levels=): a list from the coarsest level to level 0 of what the single-level mirror leaves
    -- (P, work, steps_taken, done, rows, xis, sums) -- each level started at the work of the one before it.  image and
    colors None: the geometric alignment.  keep_p: the pyramid's keep (None: the alignment's)."""
    level_steps = max_steps if level_steps is None else level_steps
    depths, images, intrs = pyramid(depth, levels, keep if keep_p is None else keep_p, image, intr)
    start = np.asarray(w2c, dtype=F32).reshape(4, 4)
    out = []
    for l in range(levels, -1, -1):
        n = max_steps if l == 0 else level_steps
        tail = (n, damping, min_used, max_rot, max_trans, eps_rot, eps_trans)
        if image is None:
            res = align.pose_align(means, start, intrs[l], depths[l], keep, beyond, kappa, near, *tail)
        else:
            res = photo.pose_align(means, colors, start, intrs[l], depths[l], images[l], keep, beyond, kappa, near, scale,
                                   max_residual, *tail)
        out.append(res)
        start = res[1]
    return out


def pose_align_batch(means, colors, w2cs, *args, **kw):
    """Per pose of w2cs [k,4,4] the list of pose_align, the level-0 entry with the batch's done word in place of the
    single call's and its sums as int64."""
    out = []
    for w2c in np.asarray(w2cs, dtype=F32).reshape(-1, 4, 4):
        per_level = pose_align(means, colors, w2c, *args, **kw)
        P, work, taken, _, hist, xis, sums = per_level[-1]
        per_level[-1] = (P, work, taken, done_of(hist), hist, xis, np.asarray(sums, dtype=np.int64))
        out.append(per_level)
    return out


# ---- the fine-textured wall -----------------------------------------------------------------------------------------
def fine_texture(P):
    """Intensity in 0.1 .. 0.9 of the world point P [..., 3] (float64): the two long waves of the wall and two of about
    0.23 m, 8.5 pixels at z = 2 with fx = 80."""
    X, Y = P[..., 0], P[..., 1]
    return (0.5 + 0.1 * np.sin(3.1 * X + 0.7 * Y) + 0.1 * np.cos(4.3 * Y - 1.3 * X) + 0.1 * np.sin(26.0 * X + 6.0 * Y)
            + 0.1 * np.cos(24.0 * Y - 7.0 * X))


def fine_wall_frame(c2w, slant=0.0, width=photo.WALL_W, height=photo.WALL_H, intr=photo.WALL_INTR):
    """tests/map_photo_ref.wall_frame with the fine texture: (depth float32 [H,W], rgb float32 [H,W,3] in 0 .. 255)."""
    fx, fy, cx, cy = intr
    v, u = np.mgrid[0:height, 0:width].astype(F64)
    dirs = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)
    c2w = np.asarray(c2w, dtype=F64)
    R, t = c2w[:3, :3], c2w[:3, 3]
    dw = dirs @ R.T
    n = np.array([-slant, 0.0, 1.0])
    lam = (2.0 - n @ t) / (dw @ n)
    grey = fine_texture(t + lam[..., None] * dw) * 255.0
    return lam.astype(F32), np.repeat(grey[..., None], 3, axis=-1).astype(F32)


def fine_move(t):
    """The truth of the basin table: 0.3 degrees about the optical axis, t metres along x and -0.6 t along y."""
    return np.array([0.0, 0.0, np.deg2rad(0.3), t, -0.6 * t, 0.0])


def fine_wall_case(t, slant=0.0):
    """The map is the frame at the identity back-projected, the query the frame at exp(fine_move(t)^); the start of the
    table is the identity.  dict(means, colors, depth, rgb, image, truth [4,4] float64 camera to world, intr)."""
    d0, rgb0 = fine_wall_frame(np.eye(4), slant)
    truth = photo.twist_pose(fine_move(t))
    d1, rgb1 = fine_wall_frame(truth, slant)
    means, colors = photo.wall_map(d0, rgb0)
    return dict(means=means, colors=colors, depth=d1, rgb=rgb1, image=photo.intensity(rgb1), truth=truth,
                intr=photo.WALL_INTR)


def coarse_wall_depth(level, slant, width=photo.WALL_W, height=photo.WALL_H, intr=photo.WALL_INTR):
    """The float64 ray-cast depth [H_l,W_l] of the wall z = 2 + slant x from the identity through the camera of a
    level: its intrinsics by the rule in float64, its pixels at the integers."""
    fx, fy, cx, cy = (float(a) for a in intr)
    for _ in range(level):
        fx, fy, cx, cy = fx * 0.5, fy * 0.5, (cx - 0.5) * 0.5, (cy - 0.5) * 0.5
    v, u = np.mgrid[0:height >> level, 0:width >> level].astype(F64)
    # z = 2 + slant x with x = (u - cx) / fx z
    return 2.0 / (1.0 - slant * (u - cx) / fx)
