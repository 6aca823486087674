"""bench.py's driver logic on the CPU (tests/bench_fake.py swaps the GPU pieces for host stand-ins): the contract of
the JSON line at N = 1, and the N = 2 path launched exactly as the harness launches it (torch.distributed.run, here
over gloo) -- strips, the per-step collective, barrier + max over ranks, rank 0 prints one line; the plain run (no
--full) that times the steps and nothing else, and the arrays --dump-outputs writes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "bench_fake.py")
SMALL = ["--gaussians", "20000", "--width", "320", "--height", "240", "--steps", "3", "--warmup", "1", "--no-graph",
         "--no-cpu-baseline", "--no-tracker", "--no-variants", "--full"]
PLAIN = ["--gaussians", "20000", "--width", "320", "--height", "240", "--warmup", "1", "--no-graph"]

REQUIRED = {"metric": str, "value": float, "unit": str, "n_gpus": int, "steps": int, "warmup": int, "ms_per_step": float,
            "higher_is_better": bool, "scaling": str, "dtype": str, "data": str, "config": dict, "roofline": dict}


def _check(line, n_gpus):
    d = json.loads(line)
    for key, typ in REQUIRED.items():
        assert isinstance(d[key], typ), (key, d[key])
    assert isinstance(d["config"]["per_frame_calibrate_ms"], float)
    assert "vs_baseline" in d and d["vs_baseline"] is None and "cpu_baseline" in d
    assert d["n_gpus"] == n_gpus and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["unit"] == "Gaussians/s" and d["scaling"] == "strong" and d["dtype"] == "f32" and d["data"] == "synthetic"
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and r["unit"] == "GB/s"
    assert set(r) >= {"achieved", "frac", "traffic", "stage_ms"} and set(r["stage_ms"]) == {
        "project_fwd", "bin", "raster_fwd", "raster_bwd", "project_bwd"}
    assert d["value"] == pytest.approx(20000 / (d["ms_per_step"] * 1e-3), rel=1e-6)
    return d


def test_single_process_line_follows_the_contract():
    res = subprocess.run([sys.executable, FAKE] + SMALL, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = _check(lines[0], 1)
    assert d["config"]["parallelism"] == "single GPU" and d["config"]["launch"] == "eager"


def test_two_ranks_as_the_harness_launches_them():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", "29533", FAKE, "--gpus", "2"] + SMALL
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]  # rank 0 only
    d = _check(lines[0], 2)
    assert d["cpu_baseline"] is None and "2 screen-tile strips" in d["config"]["parallelism"]
    assert d["config"]["strip_lists_match_full_frame_rank0"] is True
    rows = d["config"]["tile_rows_rank0"]
    assert rows[0] == 0 and 0 < rows[1] < 15  # rank 0 owns the top strip of the 15 tile rows


def test_failing_side_measurements_do_not_cost_the_headline_line():
    """Without a GPU the tracker and variant side measurements must fail -- and be reported as errors inside the
    line, next to a real cpu_baseline (the C oracle runs on the host)."""
    args = ["--gaussians", "20000", "--width", "320", "--height", "240", "--steps", "3", "--warmup", "1", "--no-graph",
            "--full"]
    res = subprocess.run([sys.executable, FAKE] + args, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = _check(lines[0], 1)
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["unit"] == "Gaussians/s" and cb["value"] > 0 and cb["cores"] >= 1
    assert "gsplat_oracle.c" in cb["sample"] and "N=20000" in cb["sample"]
    assert "error" in d["pose_opt"] and all("error" in v for v in d["variants"]) and len(d["variants"]) == 5
    assert "error" in d["api"] and "error" in d["frame"]  # (the boundary and per-frame side measurements need the GPU too)


def _run_plain(*extra, steps=3):
    res = subprocess.run([sys.executable, FAKE] + PLAIN + ["--steps", str(steps)] + list(extra), capture_output=True,
                         text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    calls = [l for l in res.stderr.splitlines() if l.startswith("[fake] forward calls ")]
    return json.loads(lines[0]), json.loads(calls[-1][len("[fake] forward calls "):])


@pytest.mark.parametrize("steps", [3, 7])
def test_plain_run_times_the_steps_and_nothing_else(steps):
    """Without --full the run sets up, warms up, times --steps steps and prints the headline: no second calibration,
    no stage timing pass, no CPU baseline, no side measurement (the forwards counted are warm-up + timed steps)."""
    d, calls = _run_plain(steps=steps)
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup"):
        assert isinstance(d[key], REQUIRED[key]), (key, d[key])
    assert d["steps"] == steps and d["warmup"] == 1 and d["unit"] == "Gaussians/s" and d["dtype"] == "f32"
    assert d["metric"].startswith("Gaussians/s fwd+bwd @20000 splats 320x240") and d["higher_is_better"] is True
    assert d["value"] == pytest.approx(20000 / (d["ms_per_step"] * 1e-3), rel=1e-6)
    assert d["step_ms_hip_events"]["n"] == steps
    assert calls == [1 + steps]
    assert "roofline" not in d and d["cpu_baseline"] is None and d["config"]["per_frame_calibrate_ms"] is None
    assert not {"parity", "pose_opt", "api", "frame", "variants"} & set(d)


def test_dump_outputs_writes_the_last_timed_step(tmp_path):
    """--dump-outputs: float32 .npy files of what the last timed step returned (the fake's image holds its forward
    count), per-Gaussian rows in the caller's order, and the same files from a second run with the same arguments."""
    dumps = []
    for run in ("a", "b"):
        d, calls = _run_plain("--dump-outputs", str(tmp_path / run), steps=4)
        assert calls == [5]
        dumps.append({f.stem: np.load(f) for f in sorted((tmp_path / run).glob("*.npy"))})
    a, b = dumps
    # (no v_quats: the benchmark's Gaussians are isotropic, their exact quaternion gradient is zero -- see dump_outputs)
    assert set(a) == {"render", "alphas", "v_viewmat", "v_means", "v_scales", "v_opacities", "v_colors"}
    assert all(v.dtype == np.float32 for v in a.values())
    assert a["render"].shape == (240, 320, 4) and (a["render"] == 5.0).all()  # written by forward 5 = the last timed step
    assert a["alphas"].shape == (240, 320, 1) and a["v_viewmat"].shape == (4, 4) and (a["v_viewmat"] == 20000).all()
    assert a["v_means"].shape == (20000, 3) and (a["v_means"][:, 0] == np.arange(20000)).all()
    assert a["v_colors"].shape == (20000, 4, 3) and a["v_opacities"].shape == (20000,)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_dump_outputs_samples_large_outputs_within_64_mb(tmp_path):
    """More Gaussians than DUMP_GAUSSIANS and an image too large for what is left: a fixed sample of each, the whole
    dump under 64 MB."""
    args = ["--gaussians", "200000", "--width", "2048", "--height", "1400", "--steps", "2", "--warmup", "1", "--no-graph",
            "--dump-outputs", str(tmp_path)]
    res = subprocess.run([sys.executable, FAKE] + args, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    files = sorted(tmp_path.glob("*.npy"))
    assert sum(f.stat().st_size for f in files) <= 64 << 20
    out = {f.stem: np.load(f) for f in files}
    rows = out["v_means"][:, 0]
    assert out["v_means"].shape == (131072, 3) and (np.diff(rows) > 0).all() and rows[-1] < 200000
    assert (out["v_scales"][:, 0] == rows).all() and (out["v_opacities"] == rows).all()
    n_pix = out["render"].shape[0]
    assert out["render"].shape == (n_pix, 4) and out["alphas"].shape == (n_pix, 1) and 0 < n_pix < 2048 * 1400
    assert (out["render"] == 3.0).all()


def test_dump_outputs_keeps_the_quaternion_gradient_of_anisotropic_gaussians(tmp_path):
    """v_quats is left out only while every Gaussian is isotropic; one anisotropic Gaussian brings it back."""
    sys.path.insert(0, ROOT)
    import torch

    import bench

    n = 10
    rows = torch.arange(n, dtype=torch.float32)
    grads = {"viewmat": torch.eye(4), "means": rows[:, None].repeat(1, 3), "quats": rows[:, None].repeat(1, 4)}
    last = {"render": torch.zeros(4, 6, 4), "alphas": torch.zeros(4, 6, 1), "grads": grads}
    ctx = type("Ctx", (), {"storage_of": None})()
    scales = torch.full((n, 3), 0.01)
    bench.dump_outputs(str(tmp_path / "iso"), last, ctx, n, scales)
    assert not (tmp_path / "iso" / "v_quats.npy").exists() and (tmp_path / "iso" / "v_means.npy").exists()
    scales[3, 1] = 0.02
    bench.dump_outputs(str(tmp_path / "aniso"), last, ctx, n, scales)
    assert (np.load(tmp_path / "aniso" / "v_quats.npy")[:, 0] == np.arange(n)).all()


def test_dump_outputs_needs_one_gpu():
    res = subprocess.run([sys.executable, FAKE, "--gpus", "2", "--dump-outputs", "unused"], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert res.returncode == 2 and "--dump-outputs needs --gpus 1" in res.stderr
