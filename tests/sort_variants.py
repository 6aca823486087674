"""Forcing one tile-sort kernel for part of a test, and proving it ran.

GSL_DEV_TILE_SORT picks the kernel on every gsl_tile_sort_keys call (include/gsloc_hip.h, gsl_tile_sort);
gsl_dev_tile_sort_launches counts, on the host, the launches of each kernel this process has issued.  A test that forces
a kernel without looking at the counters cannot tell whether the forcing took effect."""
from contextlib import contextmanager

# GSL_DEV_TILE_SORT value -> the counters of gsl_dev_tile_sort_launches it may move (0 = k_tile_sort<4>,
# 1 = k_tile_sort<5>, 2 = k_tile_sort_wg).  "wave": the wave kernel whose keys per lane the mean list length picks.
VARIANTS = {"wave16": (0,), "wave32": (1,), "wg": (2,), "wave": (0, 1)}


def launches():
    from gsplatloc_amd._lib import load_library

    lib = load_library()
    return [int(lib.gsl_dev_tile_sort_launches(v)) for v in range(3)]


def force_tile_sort(monkeypatch, kernel):
    """Set GSL_DEV_TILE_SORT=kernel; returns the launch counters to hand to assert_tile_sort_ran."""
    assert kernel in VARIANTS, kernel
    monkeypatch.setenv("GSL_DEV_TILE_SORT", kernel)
    return launches()


def assert_tile_sort_ran(kernel, before):
    """Since `before`: the forced kernel launched at least once, no other tile-sort kernel did."""
    allowed = VARIANTS[kernel]
    delta = [a - b for a, b in zip(launches(), before)]
    assert sum(delta[v] for v in allowed) >= 1, f"GSL_DEV_TILE_SORT={kernel}: the kernel never launched ({delta})"
    assert all(delta[v] == 0 for v in range(3) if v not in allowed), f"GSL_DEV_TILE_SORT={kernel}: others ran ({delta})"


@contextmanager
def forced_tile_sort(monkeypatch, kernel):
    before = force_tile_sort(monkeypatch, kernel)
    yield
    assert_tile_sort_ran(kernel, before)
