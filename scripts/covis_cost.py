#!/usr/bin/env python
"""What the covisibility kernel and a loop closure inside track() cost on the device (NOTES.md, "Loops closed in
track()").

  python scripts/covis_cost.py            # everything below, printed
  python scripts/covis_cost.py --inner spread | one   # what the profiler runs: 125 calls, nothing printed

1. `rocprofv3 --kernel-trace --stats`, a run of its own per case: 125 calls of gsl_map_covis and of gsl_map_score (one
   pose) on the same 460 800 rows -- a 640 x 480 map grown by half -- whose origins run over 48 frames ("spread"), or
   are one frame's for every row ("one": the contended word).
2. Device events around 20 calls, five windows, both cases.
3. The room loop of tests/map_correct_ref.py, tracked by a stand-in tracker that answers the drifted poses: the wall
   time of every part of the closure at frame 7 (the host synchronises in each of them), and of an attempt that ends
   ``small``.
"""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from gsplatloc_amd import _lib  # noqa: E402

W, H, ROWS, FRAMES = 640, 480, 460800, 48
INTR = (600.0, 600.0, 319.5, 239.5)
KEEP, BEYOND, NEAR = 0.95, 1.05, 0.01


def case(one: bool):
    rng = np.random.default_rng(0)
    depth = np.full((H, W), 2.0, np.float32)
    z = rng.uniform(1.8, 2.2, (ROWS, 1))
    rows = np.concatenate([rng.uniform(-0.55, 0.55, (ROWS, 1)) * z, rng.uniform(-0.42, 0.42, (ROWS, 1)) * z, z], 1)
    origins = np.full(ROWS, 7, np.int32) if one else (np.arange(ROWS) // (ROWS // FRAMES)).astype(np.int32)
    dev = "cuda"
    return dict(means=torch.from_numpy(rows.astype(np.float32)).to(dev), origins=torch.from_numpy(origins).to(dev),
                w2c=torch.eye(4).reshape(1, 16).to(dev), depth=torch.from_numpy(depth).to(dev),
                counts=torch.zeros(FRAMES, 3, dtype=torch.int32, device=dev),
                outside=torch.zeros(1, dtype=torch.int64, device=dev),
                score=torch.zeros(3, dtype=torch.int32, device=dev))


def calls(c):
    lib, ptr, st = _lib.load_library(), _lib.ptr, _lib.current_stream()

    def covis():
        _lib.check(lib.gsl_map_covis(ptr(c["means"]), ptr(c["origins"]), ROWS, ptr(c["w2c"]), *INTR, ptr(c["depth"]), W, H,
                                     KEEP, BEYOND, NEAR, FRAMES, ptr(c["counts"]), ptr(c["outside"]), st), "gsl_map_covis")

    def score():
        _lib.check(lib.gsl_map_score(ptr(c["means"]), ROWS, ptr(c["w2c"]), 1, *INTR, ptr(c["depth"]), W, H, KEEP, BEYOND,
                                     NEAR, ptr(c["score"]), st), "gsl_map_score")

    return covis, score


def inner(which):
    c = case(which == "one")
    covis, score = calls(c)
    for _ in range(125):
        covis()
        score()
    torch.cuda.synchronize()
    assert int(c["counts"].sum(0)[0]) == int(c["score"][0]) > ROWS // 2 and int(c["outside"]) == 0


def profile(which):
    rocprof = shutil.which("rocprofv3")
    if rocprof is None:
        print("rocprofv3 not found: no kernel statistics")
        return
    out = tempfile.mkdtemp(prefix="covis_prof_")
    cmd = [rocprof, "--kernel-trace", "--stats", "-d", out, "-o", "st", "--output-format", "csv", "--", sys.executable,
           os.path.abspath(__file__), "--inner", which]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if res.returncode != 0:
        print(f"{which}: profiler run failed (rc {res.returncode}): {res.stderr[-400:]}")
        return
    f = glob.glob(os.path.join(out, "**", "st_kernel_stats.csv"), recursive=True)
    rows = [r for r in csv.DictReader(open(f[0])) if "gsl::" in r["Name"]] if f else []
    shutil.rmtree(out, ignore_errors=True)
    print(f"{which}: kernel statistics, 125 calls each (rocprofv3 --kernel-trace --stats)")
    for r in sorted(rows, key=lambda r: r["Name"]):
        print("  %-28s calls %4s avg %8.2f us  min %8.2f  max %8.2f" % (
            r["Name"].replace("void gsl::", "").split("(")[0][:28], r["Calls"], float(r["AverageNs"]) / 1e3,
            float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3))


def events(which):
    c = case(which == "one")
    for name, fn in zip(("gsl_map_covis", "gsl_map_score"), calls(c)):
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
        print(f"{which}: {name}, device events around 20 calls, all its launches: "
              + ", ".join(f"{w:.1f}" for w in windows) + " us per call")


def closure():
    from gsplatloc_amd import localizer as L
    from gsplatloc_amd.mapping import MapConfig
    from gsplatloc_amd.my_gsplat import TrackerConfig
    from gsplatloc_amd.synthetic import replica_intrinsics, room_depth
    from tests import map_correct_ref as ref
    from tests import test_map_cpu as base

    w, h = 160, 120
    K = replica_intrinsics(w, h)
    true, est = ref.room_loop()
    depths = [room_depth(w, h, K, torch.from_numpy(p).float()) for p in true]
    spent = {}

    def timed(name, fn):
        def run(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **k)
            torch.cuda.synchronize()
            spent.setdefault(name, []).append((time.perf_counter() - t0) * 1e3)
            return out
        return run

    for rep in range(3):  # the first round pays for every allocation and the library's first launches
        loc = L.Localizer(K, w, h, TrackerConfig(max_steps=5), normalize=False, motion="hold", device="cuda",
                          tracker_factory=base._Tracker, mode="map",
                          map_config=MapConfig(origins=True, loop=True, loop_min_gap=7, loop_every=1))
        loc.reset(depths[0], None, torch.from_numpy(est[0]).float())
        for k in range(1, 7):
            loc.track(depths[k], None, gt_c2w=torch.from_numpy(est[k]).float())
        spent.clear()
        loc.map.covisibility = timed("covisibility", loc.map.covisibility)
        loc.map.loop_constraint = timed("loop_constraint", loc.map.loop_constraint)
        loc.map.correct = timed("correct", loc.map.correct)
        solve = L.optimise_pose_graph
        L.optimise_pose_graph = timed("optimise_pose_graph", solve)
        loc._try_loop = timed("_try_loop", loc._try_loop)
        try:
            r = loc.track(depths[7], None, gt_c2w=torch.from_numpy(est[7]).float())
            closed = {k: list(v) for k, v in spent.items()}
            spent.clear()
            at = loc.trajectory[7].cpu().double().numpy() @ np.linalg.inv(true[7]) @ true[0]
            s = loc.track(depths[0], None, gt_c2w=torch.from_numpy(at).float())
            small = {k: list(v) for k, v in spent.items()}
        finally:
            L.optimise_pose_graph = solve
        print(f"room loop, round {rep}: frame 7 {r.loop_status} ({loc.map.n_live} rows, 8 poses): "
              + ", ".join(f"{k} {' + '.join('%.2f' % v for v in vs)}" for k, vs in closed.items()) + " ms")
        print(f"room loop, round {rep}: frame 8 {s.loop_status}: "
              + ", ".join(f"{k} {' + '.join('%.2f' % v for v in vs)}" for k, vs in small.items()) + " ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", default=None, choices=["spread", "one"], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.inner:
        inner(a.inner)
        return
    for which in ("spread", "one"):
        profile(which)
    for which in ("spread", "one"):
        events(which)
    closure()


if __name__ == "__main__":
    main()
