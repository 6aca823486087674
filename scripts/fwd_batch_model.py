"""Dev tool (CPU only, numpy): a lane-level model of the compositing kernels' loop structure on workload R, to price
restructurings before anyone writes them.  60 interior tiles of the benchmark's random scene (1 M Gaussians, 1200x680,
sigma_px = 1) at the identity pose, the reference's skip (alpha < 1/255) and stop (T <= 1e-4) rules.

It first reproduces what the repository has measured on the GPU -- trust nothing else it prints unless these hold:
    forward chunk fill ~46-48 of 64, forward trips per chunk ~9.3-9.7, backward (block, entry) pairs per trip ~3.15-3.19
and then prices
    backward : block lists that run ahead across the 64-entry steps (bound: max over blocks of the summed list lengths)
    forward  : per-lane candidate queues that do not synchronise at half-chunk boundaries, spanning a chunk, a batch,
               a whole tile list
    forward  : chunks that do not restart at batch boundaries (the remainder of a batch carried into the next one)
as ratios of today's trip / chunk counts.

60 tiles (about a minute): fill 46.6, 9.38 trips per chunk, 3.25 pairs per trip (GPU, whole frame, perturbed pose:
48.5 / 9.7 / 3.15); run-ahead bound 0.926; queues 0.902 / 0.822 / 0.689; carried remainders 0.801 of the chunks.

usage: python scripts/fwd_batch_model.py [tiles]
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from gsplatloc_amd.synthetic import random_scene  # noqa: E402

N, W, H, SIGMA = 1_000_000, 1200, 680, 1.0
ALPHA_MIN, ALPHA_MAX, T_STOP = 1.0 / 255.0, 0.99, 1e-4
TAU = math.log(255.0) * 1.01 + 0.01  # r_cull: conservative radius of the alpha >= 1/255 disc (opacity 1)


def project():
    sc = random_scene(N, W, H, sigma_px=SIGMA)
    K = sc["K"].double().numpy()
    m = sc["means"].double().numpy()
    z = m[:, 2]
    u, v = K[0, 0] * m[:, 0] / z + K[0, 2], K[1, 1] * m[:, 1] / z + K[1, 2]
    cov = (K[0, 0] * sc["scales"].double().numpy()[:, 0] / z) ** 2 + 0.3
    return u, v, z, cov


def tile_list(u, v, z, cov, tx, ty):
    rad = np.ceil(3.0 * np.sqrt(cov))
    hit = ((np.floor((u - rad) / 16) <= tx) & (np.ceil((u + rad) / 16) > tx) & (np.floor((v - rad) / 16) <= ty)
           & (np.ceil((v + rad) / 16) > ty))
    idx = np.nonzero(hit)[0]
    return idx[np.argsort(z[idx], kind="stable")]


def box(c, r):
    return np.maximum(np.ceil(c - r), 0), np.minimum(np.floor(c + r), 7)


def walk_tile(u, v, cov, ids, tx, ty, st):
    """The forward's walk of one tile list; fills the counters in st and returns per quadrant the hit list
    [(entry, block nibble)]."""
    x, y, conic = u[ids], v[ids], 1.0 / cov[ids]
    rc = np.sqrt(2.0 * TAU * cov[ids])
    n = len(ids)
    lane = np.arange(64)
    hits = [[] for _ in range(4)]
    T = np.ones((4, 64))
    done = np.zeros((4, 64), bool)
    carry = [0, 0, 0, 0]  # candidates a carried remainder would hold (variant C)
    tile_cand = [[] for _ in range(4)]  # per quadrant: per-lane candidate counts per chunk half, for the queue variants
    for b0 in range(0, n, 256):
        if done.all():
            break
        sl = slice(b0, min(b0 + 256, n))
        for q in range(4):
            qx, qy = tx * 16 + 8 * (q & 1), ty * 16 + 8 * (q >> 1)
            cand = np.nonzero((np.abs(x[sl] - (qx + 4)) <= rc[sl] + 3.5) & (np.abs(y[sl] - (qy + 4)) <= rc[sl] + 3.5))[0] + b0
            st["cand"] += len(cand)
            st["chunks_all"] += (len(cand) + 63) // 64
            st["chunks_carry"] += (carry[q] + len(cand)) // 64  # full chunks only; the remainder moves on
            carry[q] = (carry[q] + len(cand)) % 64
            # lane = 16 g + p: pixel (4 (g & 1) + (p & 3), 4 (g >> 1) + (p >> 2)) of the quadrant
            g, p = lane >> 4, lane & 15
            pxl, pyl = 4 * (g & 1) + (p & 3), 4 * (g >> 1) + (p >> 2)
            batch_cnt = np.zeros(64, int)
            for c0 in range(0, len(cand), 64):
                if done[q].all():
                    break
                ch = cand[c0:c0 + 64]
                st["chunks"] += 1
                st["chunk_cand"] += len(ch)
                lox, hix = box(x[ch] - (qx + 0.5), rc[ch])
                loy, hiy = box(y[ch] - (qy + 0.5), rc[ch])
                cover = ((lox[None] <= pxl[:, None]) & (pxl[:, None] <= hix[None]) & (loy[None] <= pyl[:, None])
                         & (pyl[:, None] <= hiy[None]))  # [lane, candidate]
                comp = np.zeros((64, len(ch)), bool)
                chunk_cnt = np.zeros(64, int)
                for h0 in (0, 32):
                    cv = cover[:, h0:h0 + 32] & ~done[q][:, None]
                    if not cv.any():
                        continue
                    trips = 0
                    popped = np.zeros(64, int)
                    for ln in np.nonzero(cv.any(1))[0]:
                        k_list = np.nonzero(cv[ln])[0] + h0
                        used = 0
                        for k in k_list:
                            used += 1
                            e = ch[k]
                            dx, dy = x[e] - (qx + pxl[ln] + 0.5), y[e] - (qy + pyl[ln] + 0.5)
                            a = min(ALPHA_MAX, math.exp(-0.5 * conic[e] * (dx * dx + dy * dy)))
                            if a < ALPHA_MIN:
                                continue
                            if T[q, ln] * (1 - a) <= T_STOP:
                                done[q, ln] = True
                                break
                            T[q, ln] *= 1 - a
                            comp[ln, k] = True
                        popped[ln] = used
                        trips = max(trips, (used + 1) // 2)
                    st["trips"] += trips
                    st["pairs_fwd"] += int(popped.sum())
                    chunk_cnt += popped
                    tile_cand[q].append(popped)
                st["trips_chunk_queue"] += int(((chunk_cnt + 1) // 2).max())
                batch_cnt += chunk_cnt
                for k in np.nonzero(comp.any(0))[0]:
                    nib = 0
                    for gq in range(4):
                        if comp[16 * gq:16 * gq + 16, k].any():
                            nib |= 1 << gq
                    hits[q].append((ch[k], nib))
            st["trips_batch_queue"] += int(((batch_cnt + 1) // 2).max())
    for q in range(4):
        st["chunks_carry"] += 1 if carry[q] else 0  # (the list's last, partial chunk)
        if tile_cand[q]:
            st["trips_tile_queue"] += int(((np.sum(tile_cand[q], 0) + 1) // 2).max())
    return hits


def backward(hits, st):
    """Per quadrant: the hit list back to front in steps of 64 entries; each block walks its own entries of the step."""
    for hl in hits:
        nibs = np.array([h[1] for h in hl][::-1], int)
        tot = np.zeros(4, int)
        for s0 in range(0, len(nibs), 64):
            cnt = np.array([((nibs[s0:s0 + 64] >> g) & 1).sum() for g in range(4)])
            st["bwd_trips"] += int(cnt.max())
            st["bwd_pairs"] += int(cnt.sum())
            tot += cnt
        st["bwd_trips_bound"] += int(tot.max())


def main():
    n_tiles = int(sys.argv[1]) if len(sys.argv) > 1 else 60
    u, v, z, cov = project()
    tw, th = (W + 15) // 16, (H + 15) // 16
    rng = np.random.default_rng(0)
    tiles = [(int(rng.integers(2, tw - 2)), int(rng.integers(2, th - 3))) for _ in range(n_tiles)]
    st = dict.fromkeys(("cand", "chunks_all", "chunks_carry", "chunks", "chunk_cand", "trips", "pairs_fwd",
                        "trips_chunk_queue", "trips_batch_queue", "trips_tile_queue", "bwd_trips", "bwd_pairs",
                        "bwd_trips_bound"), 0)
    entries = 0
    for tx, ty in tiles:
        ids = tile_list(u, v, z, cov, tx, ty)
        entries += len(ids)
        backward(walk_tile(u, v, cov, ids, tx, ty, st), st)
    print(f"{n_tiles} tiles, {entries / n_tiles:.0f} entries per list")
    print(f"forward : chunk fill {st['chunk_cand'] / st['chunks']:.1f} of 64, trips per chunk {st['trips'] / st['chunks']:.2f}, "
          f"(pixel, candidate) pairs per trip {st['pairs_fwd'] / st['trips']:.1f} of 128")
    print(f"backward: (block, entry) pairs per trip {st['bwd_pairs'] / st['bwd_trips']:.2f} of 4")
    print(f"backward, block lists running ahead across steps (bound): trips x {st['bwd_trips_bound'] / st['bwd_trips']:.3f}")
    for k, name in (("trips_chunk_queue", "a 64-candidate chunk"), ("trips_batch_queue", "a whole batch"),
                    ("trips_tile_queue", "a whole tile list")):
        print(f"forward, per-lane queue spanning {name}: trips x {st[k] / st['trips']:.3f}")
    print(f"forward, chunks that do not restart at batch boundaries: chunks x {st['chunks_carry'] / st['chunks_all']:.3f} "
          f"(no early termination in either count)")


if __name__ == "__main__":
    main()
