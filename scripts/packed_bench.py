"""Dev tool: the packed pipeline (packed=True with GSLOC_PACKED=1, or sparse_grad=True) against the staged dense path
(GSLOC_DISABLE_FUSED=1, GSLOC_PACKED unset), one rasterization() forward + backward ("RGB+ED", SH degree 1, gradients of
the Gaussians and of the poses), 1 M Gaussians, 640x480:

  (a) four cameras over a cloud five times as wide as a frustum: at most a tenth of the (camera, Gaussian) pairs visible;
  (b) one camera that sees everything.

Per-step HIP events after a warm-up, as bench.py times; the variants alternate step by step inside one process, median
and the 10th..90th percentile spread are printed.  bench.py's headline (fused one-camera path) does not come here.

    python scripts/packed_bench.py [--steps 20] [--warmup 5] [--n 1000000] [--out profiles/packed_bench.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = (("staged dense", "0", False), ("packed, dense gradients", "1", False), ("packed, sparse gradients", "0", True))


def scenes(N, W, H):
    import torch

    from gsplatloc_amd.synthetic import perturbed_pose, random_scene

    for name, C, spread in (("a: C=4, cloud 5x the frustum", 4, 5.0), ("b: C=1, everything visible", 1, 1.0)):
        sc = random_scene(N, W, H, device="cuda")
        sc["means"][:, :2] *= spread
        Vs = torch.stack([torch.linalg.inv(perturbed_pose(0.5 + c, 0.01 + 0.02 * c, seed=7 + c)) for c in range(C)]).cuda()
        yield name, C, sc, Vs


def step_fn(sc, Vs, W, H, env, sparse):
    import torch

    import gsplatloc_amd as A

    C = Vs.shape[0]
    Ks = sc["K"][None].expand(C, 3, 3).contiguous()
    v = torch.randn(C, H, W, generator=torch.Generator().manual_seed(1)).cuda()
    share = []

    def step():
        os.environ["GSLOC_PACKED"] = env
        Vg = Vs.clone().requires_grad_()
        ins = [sc[k].clone().requires_grad_() for k in ("means", "quats", "scales", "opacities", "sh")]
        beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        beg.record()
        rc, ra, meta = A.rasterization(*ins, viewmats=Vg, Ks=Ks, width=W, height=H, sh_degree=1, packed=True,
                                       sparse_grad=sparse, render_mode="RGB+ED")
        (rc[..., 3] * v).sum().backward()
        end.record()
        if not share:
            ids = meta["camera_ids"]
            share.append((ids.numel() if ids is not None else int((meta["radii"] > 0).sum())) / (C * sc["means"].shape[0]))
        return beg, end

    return step, share


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, metavar="SCENE:VARIANT",
                    help="e.g. b:1 -- run only that scene (a, b) and variant (0, 1, 2), untimed: the program to put "
                         "after `rocprofv3 --kernel-trace --stats --`")
    a = ap.parse_args()
    os.environ["GSLOC_DISABLE_FUSED"] = "1"
    W, H = 640, 480
    if a.only:
        which, k = a.only.split(":")
        for name, C, sc, Vs in scenes(a.n, W, H):
            if name.startswith(which):
                step, _ = step_fn(sc, Vs, W, H, *VARIANTS[int(k)][1:])
                for _ in range(a.warmup + a.steps):
                    step()
                torch.cuda.synchronize()
        return
    lines = []
    for name, C, sc, Vs in scenes(a.n, W, H):
        steps = [step_fn(sc, Vs, W, H, env, sparse) for _, env, sparse in VARIANTS]
        events = [[] for _ in VARIANTS]
        for it in range(a.warmup + a.steps):
            for k, (step, _) in enumerate(steps):  # the variants alternate
                ev = step()
                if it >= a.warmup:
                    events[k].append(ev)
        torch.cuda.synchronize()
        lines.append(f"{name}: N={a.n} {W}x{H}, visible share of the pairs {steps[0][1][0]:.3f}, {a.steps} steps each")
        med = []
        for (label, _, _), evs in zip(VARIANTS, events):
            ms = sorted(b.elapsed_time(e) for b, e in evs)
            q = lambda f: ms[min(len(ms) - 1, int(f * len(ms)))]  # noqa: E731
            med.append(q(0.5))
            lines.append(f"  {label:26s} fwd+bwd median {q(0.5):8.3f} ms  (10%..90%: {q(0.1):.3f} .. {q(0.9):.3f})"
                         + ("" if len(med) == 1 else f"  = {med[-1] / med[0]:.2f} x staged dense"))
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
