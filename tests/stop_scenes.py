"""Constructed "stop ladder" scenes for the compositing forward's per-pixel decisions (inputs only; tests/walk_ref.py walks
them, tests/test_walk_ref_cpu.py shows that every case below is really present, tests/test_gpu_fwd_decisions.py runs them).

Small images whose tiles each carry one case, seen from the identity pose; list order is set through strictly increasing
depths (1 + 0.001 x position), the Gaussians themselves are stored in a shuffled order.  Every Gaussian keeps its tile
rectangle (7 px for the fillers and stoppers, 4 px for the dots -- the radius rule floors the eigenvalue gap at 0.1 px^2 -- around
a centre near the tile's middle) inside ONE tile, so a tile's list is exactly what
its spec says, and every "filler", "stopper" and "dot" placed in the tile's middle is a candidate of all four quadrants:
candidate position = list position within the 256-record batch (asserted on the CPU).  Three kinds of entries:

  fillers   sigma 2.2 px at the tile's middle (8, 8) -- between the pixel centres, so a pixel's squared distance is one
            of 0.5, 2.5, 4.5, ... -- with an opacity from four classes chosen so that alpha / (1/255) stays more than 3 %
            from 1 at every such distance (0.0045, 0.0065, 0.0095, 0.014), and in the long lists "ghosts" of opacity 0.003
            that never reach 1/255: they lengthen the list, not the candidate lists;
  dot pairs sigma 0.8 px, opacity 1.0, centred exactly on a TARGET pixel: alpha is clamped at 0.999 there, the first dot
            (early in the list) leaves T = F x 0.001 > 1e-4, and the second one, at list position p, stops the pixel AT p:
            T x 0.001 <= 1e-4.  The four targets of a tile are 5 px apart, one per quadrant, and do not see each other's
            dots (alpha < 1/255 at 5 px).  Without the clamp the first dot would stop the pixel;
  stoppers  sigma 2.2 px, opacity 0.9, jittered by 0.4 px, in a run of a dozen: the pixels of a wave stop on DIFFERENT
            entries of the run (the spread is asserted), which the run places across a chunk, batch or segment seam.

Tiles of the ragged image (56x40: the last column is 8 px wide, the last row 8 px high) use the same entries at sigma
1.1 px around (4.2, 4.2).

Condition on the scenes: on the records of the float32 oracle projection -- plain and rounded as an fp16-staged record
rounds them -- no decision of any pixel has a margin below CPU_MARGIN (2e-3); the GPU test asserts 1e-3 on the records the
forward actually used.  _settle() reaches it by nudging the opacity of an offending Gaussian by 1 % until the reference
reports the margin; no outlier is allowed anywhere.
"""
import functools

import numpy as np
import torch

from tests import walk_ref as WR

FX = 200.0
CPU_MARGIN = 2e-3
GPU_MARGIN = 1e-3
CLASSES = (0.0045, 0.0065, 0.0095, 0.014)
GHOST = 0.003
Q4 = ((5, 5), (10, 5), (5, 10), (10, 10))  # one target pixel per quadrant, 5 px apart


def _t(*positions, firsts=None):
    return [dict(p=p, pixel=Q4[i], first=(firsts[i] if firsts else i)) for i, p in enumerate(positions)]


SHORT = {
    (0, 0): dict(n=12, targets=[dict(p=1, pixel=(8, 8), first=0)]),           # the second of two alpha 0.999 entries
    (1, 0): dict(n=60, targets=_t(30, 31, 32, 33)),
    (2, 0): dict(n=90, targets=_t(62, 63, 64, 65)),
    (3, 0): dict(n=290, targets=_t(127, 128, 255, 256)),
    (0, 1): dict(n=300, targets=_t(257, 299)),                                # 299: the last entry of the list
    (1, 1): dict(n=37),                                                       # never stops; an odd candidate count
    # (2, 1): blank
    (3, 1): dict(n=1, faint=True),                                            # one contribution, alpha just above 1/255
    (0, 2): dict(n=41, strong=(20, 12), dots=4),
    (1, 2): dict(n=80, strong=(58, 12)),                                      # across the chunk seam at 64
    (2, 2): dict(n=275, strong=(250, 12)),                                    # across the batch seam at 256
    (3, 2): dict(n=61, dots=40),
}
_C = dict(compact=True)
RAGGED = {
    (0, 0): dict(n=60, targets=_t(30, 31, 32, 33)),
    (1, 0): dict(n=90, targets=_t(62, 63, 64, 65)),
    (2, 0): dict(n=41, strong=(20, 12), dots=4),
    (3, 0): dict(n=40, targets=[dict(p=31, pixel=(4, 4), first=0)], **_C),
    (0, 1): dict(n=290, targets=_t(127, 128, 255, 256)),
    (1, 1): dict(n=37),
    (2, 1): dict(n=12, targets=[dict(p=1, pixel=(8, 8), first=0)]),
    (3, 1): dict(n=30, strong=(15, 8), **_C),
    (0, 2): dict(n=70, targets=[dict(p=64, pixel=(4, 4), first=0)], **_C),
    # (1, 2): blank
    (2, 2): dict(n=1, faint=True, **_C),
    (3, 2): dict(n=20, targets=[dict(p=19, pixel=(4, 4), first=0)], **_C),    # the corner tile: 8 x 8 pixels
}
_S = dict(n=3)
_short10 = lambda skip: {(tx, ty): dict(_S) for ty in range(3) for tx in range(4) if (tx, ty) not in skip}  # noqa: E731
# long lists (2049 .. 2700 entries; segments of 128): L = 2600 has 21 segments, quarters of 6; L = 2177 and 2300 have 18,
# quarters of 5; L = 2049 and 2100 have 17, quarters of 5
LONG_A = {**_short10(((0, 0), (2, 1))),
          (0, 0): dict(n=2600, ghosts=0.7, targets=_t(383, 384, 385, 5)),     # 128 k - 1, 128 k, 128 k + 1; segment 0
          (2, 1): dict(n=2600, ghosts=0.7, targets=_t(767, 768, 1023, 1024))}  # quarter seam (6 x 128); segments 7 / 8
LONG_B = {**_short10(((1, 0), (3, 2))),
          (1, 0): dict(n=2177, ghosts=0.7, targets=_t(2176, 639, 640, 1920)),  # the very last entry; quarter seams
          (3, 2): dict(n=2049, ghosts=0.7, early=(3, (4, 4)))}                 # never stops; an early entry and no more
LONG_C = {**_short10(((0, 1), (2, 2))),
          (0, 1): dict(n=2300, ghosts=0.7, strong=(1272, 16)),                 # across segments 9 / 10 = a quarter seam
          (2, 2): dict(n=2100, ghosts=0.7, strong=(120, 16))}                  # across segments 0 / 1
SCENES = {"short": (64, 48, SHORT), "ragged": (56, 40, RAGGED), "long-a": (64, 48, LONG_A), "long-b": (64, 48, LONG_B),
          "long-c": (64, 48, LONG_C)}
LONG_SCENES = ("long-a", "long-b", "long-c")


def _tile_entries(spec, rng):
    """The tile's list, front to back: rows (u, v, sigma, opacity) relative to the tile's origin."""
    n = spec["n"]
    compact = spec.get("compact", False)
    mid, sig = (4.2, 1.1) if compact else (8.0, 2.2)  # (4.2: the rectangle 4.2 +- 4 stays off the tile's border)
    rows = [None] * n
    if spec.get("faint"):
        return [(mid + 0.5, mid + 0.5, sig, 0.0041)]
    for t in spec.get("targets", ()):
        u, v = t["pixel"][0] + 0.5, t["pixel"][1] + 0.5
        rows[t["first"]] = (u, v, 0.8, 1.0)
        rows[t["p"]] = (u, v, 0.8, 1.0)
    if "strong" in spec:
        s, c = spec["strong"]
        for k in range(s, s + c):
            lo = 0.0 if compact else -0.4  # (compact: a centre left of or above the middle would reach the neighbour tile)
            rows[k] = (mid + rng.uniform(lo, 0.4), mid + rng.uniform(lo, 0.4), sig, 0.9)
    if "early" in spec:
        k, (i, j) = spec["early"]
        rows[k] = (i + 0.5, j + 0.5, 0.8, 0.5)
    free = [k for k in range(n) if rows[k] is None]
    for k in rng.choice(free, size=min(spec.get("dots", 0), len(free)), replace=False):
        rows[k] = (rng.uniform(5.3, 10.7), rng.uniform(5.3, 10.7), rng.uniform(0.6, 1.0), rng.uniform(0.3, 0.9))
    for k in range(n):
        if rows[k] is None:
            # behind a run of stoppers in a long list only ghosts: a pixel the run left just above 1e-4 would otherwise
            # creep onto the threshold in steps of 0.4 %
            behind = "strong" in spec and "ghosts" in spec and k > spec["strong"][0]
            ghost = behind or rng.uniform() < spec.get("ghosts", 0.0)
            rows[k] = (mid, mid, sig, GHOST if ghost else CLASSES[int(rng.integers(0, len(CLASSES)))])
    return rows


def _settle(sc, tiles):
    """Nudge opacities by 1 % until no pixel of any tile takes a decision within CPU_MARGIN of a threshold, on the plain
    and on the half-rounded records."""
    recs = [WR.records_from_oracle(sc, "ED", half) for half in (False, True)]
    op = sc["opacities"].double().numpy().copy()
    tw = (sc["W"] + 15) // 16
    nudged = 0
    for (tx, ty) in tiles:
        t = ty * tw + tx
        for _ in range(60):
            bad = set()
            for (rec, offs, flat), half in zip(recs, (False, True)):
                rec["op"] = torch.from_numpy(op).float().half().double().numpy() if half else op.astype(np.float32).astype(np.float64)
                rs, re = int(offs[t]), int(offs[t + 1])
                px, py = WR.tile_pixels(tx, ty)
                act = (px < sc["W"]) & (py < sc["H"])
                res = WR.walk(rec, flat[rs:re], px, py, act, keep_below=1.25 * CPU_MARGIN)
                for kind, p, k, _m in res["near"]:
                    g = int(flat[rs + k])
                    if kind == "T" and op[g] < 0.05:  # a thin entry cannot move T: the strongest one in front of it can
                        seen = [int(flat[rs + kk]) for kk in np.nonzero(res["comp"][p, :k])[0]]
                        pick = [x for x in seen if op[x] < 0.999] or seen or [g]
                        g = max(pick, key=lambda x: op[x])
                    bad.add(g)
            if not bad:
                break
            for g in bad:
                op[g] *= 0.99 if op[g] > 0.95 else 1.01
            nudged += len(bad)
        else:
            raise AssertionError(f"scene too close to a threshold: tile ({tx}, {ty}) does not settle")
    sc["opacities"] = torch.from_numpy(op).float().contiguous()
    return nudged


@functools.lru_cache(maxsize=None)
def scene(name):
    """float32 inputs of a scene: means, quats, scales, opacities, rgb [N, 3] (colours as they are: sh_degree None), V, K;
    W, H, N, tiles (the specs) and nudged (how many 1 % nudges the condition took)."""
    W, H, tiles = SCENES[name]
    rng = np.random.default_rng(sorted(SCENES).index(name) + 20)
    U, V, S, O = [], [], [], []
    for (tx, ty), spec in tiles.items():
        for u, v, s, o in _tile_entries(spec, rng):
            U.append(16.0 * tx + u)
            V.append(16.0 * ty + v)
            S.append(s)
            O.append(o)
    N = len(U)
    u, v, s, o = (torch.tensor(t, dtype=torch.float64) for t in (U, V, S, O))
    z = 1.0 + 1e-3 * torch.arange(N, dtype=torch.float64)
    cx, cy = W / 2.0, H / 2.0
    means = torch.stack([(u - cx) / FX * z, (v - cy) / FX * z, z], -1)
    scales = (s * z / FX)[:, None].repeat(1, 3)
    quats = torch.tensor([1.0, 0, 0, 0], dtype=torch.float64).repeat(N, 1)
    g = torch.Generator().manual_seed(5)
    perm = torch.randperm(N, generator=g)
    f32 = lambda t: t[perm].float().contiguous()  # noqa: E731
    sc = dict(means=f32(means), quats=f32(quats), scales=f32(scales), opacities=f32(o),
              rgb=torch.rand(N, 3, generator=g).contiguous(), V=torch.eye(4), W=W, H=H, N=N, tiles=tiles,
              K=torch.tensor([[FX, 0, cx], [0, FX, cy], [0, 0, 1]], dtype=torch.float32))
    sc["nudged"] = _settle(sc, list(tiles))
    return sc


def inputs(sc, mode, device):
    """The seven arguments of RenderContext.calibrate / forward."""
    rgb = sc["rgb"].to(device) if mode.startswith("RGB") else None
    return [sc[k].to(device) for k in ("means", "quats", "scales", "opacities")] + [rgb, sc["V"].to(device), sc["K"].to(device)]
