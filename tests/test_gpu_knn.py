"""GPU: csrc/knn.hip (uniform 128^3 grid, shell search) against scipy's cKDTree in float64 on the float32 points, at
the clouds that stress the search's termination rule -- it ends when best[k-1] <= reach^2 or when the whole grid has
been covered: every k template edge, clouds smaller than k, clouds that collapse the grid to a cell, a line or a
plane, far outliers that squeeze everything else into one cell, and coordinates far from the origin."""
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
RTOL, ATOL = 2e-5, 1e-10  # the bound of test_device_knn_matches_kdtree, on SQUARED distances


def _random_cloud(n=5000):
    """the `random` cloud of test_device_knn_matches_kdtree, cut to n points"""
    g = torch.Generator().manual_seed(3)
    pts = torch.rand(20000, 3, generator=g) * torch.tensor([4.0, 0.3, 2.0]) + torch.tensor([-1.0, 5.0, 0.0])
    return pts[:n].contiguous()


def _reference(pts, k):
    """squared distances [N,k] of the exact k nearest neighbours (self included); +inf where there are fewer than k"""
    from scipy.spatial import cKDTree
    p = pts.double().numpy()
    d, _ = cKDTree(p).query(p, k=k)
    return np.asarray(d, dtype=np.float64).reshape(len(p), k) ** 2


def _check(pts, k, tag):
    from gsplatloc_amd.my_gsplat.utils import knn_device
    ref = _reference(pts, k)
    x = pts.to(DEV)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    d2 = knn_device(x, k)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert d2.shape == (pts.shape[0], k) and d2.dtype == torch.float32
    got = d2.cpu().double().numpy()
    finite = np.isfinite(ref) & (ref > 0)
    err = float(np.max(np.abs(got[finite] - ref[finite]) / ref[finite])) if finite.any() else 0.0
    print(f"[knn] {tag}: N={pts.shape[0]} k={k}: {dt * 1e3:.1f} ms, largest relative error {err:.1e} (<= {RTOL:.0e})")
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL)  # equal infinities count as equal
    return got


@pytest.mark.parametrize("k", [1, 2, 8])
def test_knn_smallest_and_largest_k(k):
    _check(_random_cloud(), k, "random")


@pytest.mark.parametrize("k", [8, 4])
@pytest.mark.parametrize("N", [1, 3, 8, 255, 256, 257])
def test_knn_small_clouds(N, k):
    """One block, one block and a thread, and clouds with fewer points than neighbours asked for: the missing
    neighbours are +inf on the device as on the host path of utils.knn (the search then ends on the whole-grid rule)."""
    from gsplatloc_amd.my_gsplat.utils import knn
    pts = torch.rand(N, 3, generator=torch.Generator().manual_seed(40 + N))
    got = _check(pts, k, "unit cube")
    assert np.isinf(got[:, min(N, k):]).all() and np.isfinite(got[:, :min(N, k)]).all()
    ref = _reference(pts, k)
    for dev in ("cpu", DEV):
        d2 = knn(pts.to(dev), k)
        assert d2.device.type == torch.device(dev).type and d2.shape == (N, k)
        np.testing.assert_allclose(d2.cpu().double().numpy(), ref, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("case", ["identical", "line", "plane", "two_clusters"])
def test_knn_collapsed_grids(case):
    """Bounding boxes with no extent in three, two or one direction, and one that is empty but for two corners."""
    N, k = 2000, 5
    g = torch.Generator().manual_seed(7)
    if case == "identical":
        pts = torch.tensor([0.3, -1.2, 2.5]).repeat(N, 1)
    elif case == "line":
        pts = torch.zeros(N, 3) + torch.tensor([0.0, 1.5, -0.5])
        pts[:, 0] = torch.rand(N, generator=g) * 10.0
    elif case == "plane":
        pts = torch.rand(N, 3, generator=g) * torch.tensor([3.0, 2.0, 0.0]) + torch.tensor([0.0, 0.0, 2.0])
    else:
        pts = torch.rand(N, 3, generator=g) * 0.01
        pts[N // 2:] += torch.tensor([50.0, 0.0, 0.0])
    got = _check(pts, k, case)
    if case == "identical":
        assert (got == 0.0).all()


def test_knn_far_outliers():
    """3000 points in a 1 cm cube and two points at opposite corners of a 200 m cube around it: the cluster falls
    into ONE cell of 1.57 m, each of its points scans that cell; the outliers sit in corner cells and expand their
    search for 110 shells until 110 h >= 173 m, the distance to the cluster (reach rule; the grid clips the shells)."""
    g = torch.Generator().manual_seed(8)
    centre = torch.tensor([1000.0, -3.0, 7.0])
    cluster = centre + (torch.rand(3000, 3, generator=g) - 0.5) * 0.01
    pts = torch.cat([cluster, (centre - 100.0)[None], (centre + 100.0)[None]]).contiguous()
    lo = pts.double().amin(0)
    h = float((pts.double().amax(0) - lo).max()) / 127.0 * 1.0001
    cells = torch.floor((pts.double() - lo) / h)
    assert len(torch.unique(cells[:3000], dim=0)) == 1  # (mid-cell: float32 rounding of the kernel's own h cannot split it)
    assert cells[3000].tolist() == [0.0, 0.0, 0.0] and float(cells[3001].min()) >= 126.0
    got = _check(pts, 8, "far outliers")
    assert got[3000, 0] == 0.0 and abs(got[3000, 1] - 3.0e4) < 0.01 * 3.0e4  # ~100 sqrt(3) m to the cluster


def test_knn_far_from_the_origin():
    """Coordinates of a few thousand (metres of a large scene): float32 spacing 1.2e-4 at 2000, cell size ~3 cm."""
    pts = (_random_cloud(20000) + torch.tensor([2000.0, -1500.0, 800.0])).contiguous()
    _check(pts, 5, "shifted")
