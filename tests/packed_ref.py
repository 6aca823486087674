"""What packed mode must return, composed from DENSE results (test code only; the oracle and the dense path stay
dense): the rows of the [C,N,...] tensors at nonzero(radii > 0), in row-major order, i.e. ascending camera * N +
gaussian."""
import torch


def pack_rows(t, radii):
    """Rows of t [C,N,...] where radii [C,N] > 0, row-major."""
    return t[radii > 0]


def pack(dense):
    """dense = (radii [C,N], means2d [C,N,2], depths [C,N], conics [C,N,3], compensations [C,N] | None), the return
    of a dense fully_fused_projection -> dict of the packed call's seven results."""
    radii, means2d, depths, conics, comps = dense
    ids = torch.nonzero(radii > 0)  # [nnz, 2], sorted lexicographically (row-major)
    return dict(camera_ids=ids[:, 0].to(torch.int64), gaussian_ids=ids[:, 1].to(torch.int64),
                radii=pack_rows(radii, radii), means2d=pack_rows(means2d, radii), depths=pack_rows(depths, radii),
                conics=pack_rows(conics, radii), compensations=None if comps is None else pack_rows(comps, radii))


NAMES = ("camera_ids", "gaussian_ids", "radii", "means2d", "depths", "conics", "compensations")


def as_dict(packed):
    """The seven-tuple of fully_fused_projection(packed=True) under the names above."""
    return dict(zip(NAMES, packed))
