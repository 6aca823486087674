#!/usr/bin/env python
"""What occlusion culling of the local map costs on the device ("Occlusion culling"; NOTES.md).

  python scripts/occl_cost.py [--lib PATH ...]      # everything below, printed, for the library and every PATH
  python scripts/occl_cost.py --inner raster|random [--lib PATH]   # what the profiler runs: 125 calls, nothing printed

`rocprofv3 --kernel-trace --stats`, a run of its own per case and library: 125 calls each of gsl_map_view_select (the
frustum alone), gsl_map_occl_depth and gsl_map_occl_select on the same 460 800 rows, then device events around 20 calls.
  raster  a 640 x 480 map grown by half: a frame's pixels in raster order -- a room with a panel in front of its back
          wall -- and the upper half of a second view 10 cm to the right, selected from the first pose.  Neighbouring
          lanes fall into the same cell: the contended case.
  random  the rows of scripts/covis_cost.py, depths 1.8 .. 2.2 m all over the image: neighbouring lanes fall into
          cells far apart, and most rows lie behind another one.
--lib: a library built with another variant of the depth kernel, e.g.
  make -C gsplatloc_amd/csrc EXTRA="-DGSL_OCCL_PRELOAD=0 -DGSL_OCCL_COMBINE=1"
into a copy of the tree (the kernel's name carries the two template arguments)."""
import argparse
import csv
import ctypes
import glob
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from gsplatloc_amd import _lib  # noqa: E402
from gsplatloc_amd.synthetic import panel_depth  # noqa: E402

W, H, ROWS = 640, 480, 460800
INTR = (600.0, 600.0, 319.5, 239.5)
NEAR, FAR, GUARD, CELL, WINDOW, KEEP = 0.01, 1e10, 8.0, 4, 1, 0.95


def library(path):
    if path is None:
        return _lib.load_library()
    lib = ctypes.CDLL(os.path.abspath(path))
    for name in ("gsl_map_view_ws_bytes", "gsl_map_view_select", "gsl_map_occl_ws_bytes", "gsl_map_occl_zbuf_bytes",
                 "gsl_map_occl_depth", "gsl_map_occl_select"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib._SIGNATURES[name]
    return lib


def case(which):
    if which == "random":
        rng = np.random.default_rng(0)
        z = rng.uniform(1.8, 2.2, (ROWS, 1))
        rows = np.concatenate([rng.uniform(-0.55, 0.55, (ROWS, 1)) * z, rng.uniform(-0.42, 0.42, (ROWS, 1)) * z, z], 1)
    else:
        K = torch.tensor([[INTR[0], 0.0, INTR[2]], [0.0, INTR[1], INTR[3]], [0.0, 0.0, 1.0]])
        v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        rows = []
        for x, count in ((0.0, W * H), (0.1, ROWS - W * H)):
            c2w = torch.eye(4)
            c2w[0, 3] = x
            d = panel_depth(W, H, K, c2w, center=(0.0, 0.0), size=(0.8, 0.6), z=1.0).double().numpy()
            p = np.stack([(u - INTR[2]) / INTR[0] * d + x, (v - INTR[3]) / INTR[1] * d, d], -1).reshape(-1, 3)
            rows.append(p[:count])
        rows = np.concatenate(rows)
    assert rows.shape == (ROWS, 3)
    dev = "cuda"
    return dict(means=torch.from_numpy(rows.astype(np.float32)).to(dev), w2c=torch.eye(4).reshape(1, 16).to(dev))


def calls(c, lib):
    ptr, st, dev = _lib.ptr, _lib.current_stream(), "cuda"
    view_ws = torch.empty(lib.gsl_map_view_ws_bytes(ROWS), dtype=torch.uint8, device=dev)
    ws = torch.empty(lib.gsl_map_occl_ws_bytes(ROWS), dtype=torch.uint8, device=dev)
    z_bytes = lib.gsl_map_occl_zbuf_bytes(W, H, GUARD, CELL)
    zbuf = torch.zeros(z_bytes // 4, dtype=torch.int32, device=dev)
    c["view_counters"] = torch.zeros(3, dtype=torch.int32, device=dev)
    c["counters"] = torch.zeros(4, dtype=torch.int32, device=dev)
    c["zbuf"] = zbuf

    def view():
        _lib.check(lib.gsl_map_view_select(ptr(c["means"]), ROWS, ptr(c["w2c"]), *INTR, W, H, GUARD, NEAR, FAR, None,
                                           ptr(c["view_counters"]), ptr(view_ws), view_ws.numel(), st),
                   "gsl_map_view_select")

    def depth():
        _lib.check(lib.gsl_map_occl_depth(ptr(c["means"]), ROWS, ptr(c["w2c"]), *INTR, W, H, GUARD, CELL, NEAR, FAR,
                                          ptr(zbuf), z_bytes, st), "gsl_map_occl_depth")

    def select():
        _lib.check(lib.gsl_map_occl_select(ptr(c["means"]), ROWS, ptr(c["w2c"]), *INTR, W, H, GUARD, NEAR, FAR, CELL,
                                           WINDOW, KEEP, ptr(zbuf), z_bytes, None, ptr(c["counters"]), ptr(ws),
                                           ws.numel(), st), "gsl_map_occl_select")

    return view, depth, select


def inner(which, path):
    c = case(which)
    view, depth, select = calls(c, library(path))
    for _ in range(125):
        view()
        depth()
        select()
    torch.cuda.synchronize()
    in_view, (selected, _, _, culled) = int(c["view_counters"][0]), c["counters"].tolist()
    assert selected + culled == in_view > ROWS // 2 and culled > 0, (in_view, selected, culled)
    print(f"{which}: {in_view} rows in the band, {culled} culled, {int((c['zbuf'] != 0).sum())} cells hold a row")


def profile(which, path):
    rocprof = shutil.which("rocprofv3")
    if rocprof is None:
        print("rocprofv3 not found: no kernel statistics")
        return
    out = tempfile.mkdtemp(prefix="occl_prof_")
    cmd = [rocprof, "--kernel-trace", "--stats", "-d", out, "-o", "st", "--output-format", "csv", "--", sys.executable,
           os.path.abspath(__file__), "--inner", which] + (["--lib", path] if path else [])
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if res.returncode != 0:
        print(f"{which}: profiler run failed (rc {res.returncode}): {res.stderr[-400:]}")
        return
    f = glob.glob(os.path.join(out, "**", "st_kernel_stats.csv"), recursive=True)
    rows = [r for r in csv.DictReader(open(f[0])) if "gsl::" in r["Name"]] if f else []
    shutil.rmtree(out, ignore_errors=True)
    print(f"{which}, {path or 'the library'}: kernel statistics, 125 calls each (rocprofv3 --kernel-trace --stats); "
          + res.stdout.strip().splitlines()[-1])
    for r in sorted(rows, key=lambda r: r["Name"]):
        print("  %-44s calls %4s avg %8.2f us  min %8.2f  max %8.2f" % (
            r["Name"].replace("void gsl::", "").split("(")[0][:44], r["Calls"], float(r["AverageNs"]) / 1e3,
            float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3))


def events(which, path):
    c = case(which)
    for name, fn in zip(("gsl_map_view_select", "gsl_map_occl_depth", "gsl_map_occl_select"), calls(c, library(path))):
        for _ in range(3):
            fn()
        windows = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(20):
                fn()
            b.record()
            torch.cuda.synchronize()
            windows.append(a.elapsed_time(b) * 1e3 / 20)
        print(f"{which}, {path or 'the library'}: {name}, device events around 20 calls, all its launches: "
              + ", ".join(f"{w:.1f}" for w in windows) + " us per call")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", default=None, choices=["raster", "random"], help=argparse.SUPPRESS)
    ap.add_argument("--lib", action="append", default=[], help="another build of the library to measure as well")
    a = ap.parse_args()
    if a.inner:
        inner(a.inner, a.lib[0] if a.lib else None)
        return
    for path in [None] + a.lib:
        for which in ("raster", "random"):
            profile(which, path)
    for path in [None] + a.lib:
        for which in ("raster", "random"):
            events(which, path)


if __name__ == "__main__":
    main()
