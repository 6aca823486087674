"""Record-level reference of the compositing walk (test code only, numpy; nothing here is part of oracle/).

The compositing forward takes three discrete decisions per (pixel, list entry): it skips an entry whose alpha is below
1/255, clamps alpha at 0.999, and stops the pixel BEFORE an entry that would bring T to 1e-4 or below; then it records the
list index of the last entry it composited.  walk() restates that loop in float64 on the per-Gaussian RECORDS exactly as
the kernels read them (centre, conic, effective opacity, features) and on one tile list in order, for the 256 pixels of
the tile, and returns what the pixel ended with, where it stopped, what it composited, and how far every decision it took
was from flipping:

  margin_alpha  the smallest |alpha / ALPHA_MIN - 1| over the entries the pixel reached with sigma >= 0
  margin_T      the smallest |T_next / T_STOP - 1| over the entries it composited or stopped on

The cull radius is deliberately not an input of the decisions: the reference applies the alpha rule to every entry, so a
radius that is too small shows as a difference.  (A record's radius is read only by the mutants that model a defect of the
candidate lists: cull98, skip32, pair_second.)

`force` flips chosen (pixel, entry) decisions -- ("alpha", pixel, entry) or ("T", pixel, entry) -- which is what lets a
test EXPLAIN a pixel that differs: it must equal the walk with a few near-threshold decisions forced the other way.

`mutant` names a deliberately wrong walk (MUTANTS); tests/test_walk_ref_cpu.py shows that the comparator of the GPU test
rejects every one of them.

frame_reference() runs the walk over every tile of a frame and lays the results out as the kernels write them: render
(expected depth divided by max(alpha, 1e-10)), alphas = 1 - T, last_ids (absolute list index, 0 when nothing was
composited) and, per quadrant, the hit list ((bits of the 4x4 blocks that composited the entry) << 28 | absolute list
index, in list order: the layout documented at isect_hits in praster_walk, gsplatloc_amd/csrc/raster_px.hip).
compare_frames() is the comparator: every pixel, no allowance.

Error model behind DELTA (the margin below which a float32 kernel and this reference may legitimately take a decision
differently), first order, eps = 2^-24 (half an ulp, relative):
  * alpha leg: log2(e) sigma = fma(b' dx, dy, fma(a' dx, dx, c' dy dy)) on staged a', b', c' -- the two subtractions, the
    three staging products and the six rounded operations of the expression are at most 11 roundings of terms no larger
    than the result's magnitude bound, 8 in log2 units where alpha can still reach 1/255 from opacity 1 (2^-8 = 1/256):
    |d sigma_log2| <= 11 eps 8, which exp2 turns into a relative error ln 2 x that = 3.6e-6; exp2 itself is good to one
    ulp (2 eps) and the product with the opacity rounds once more (eps): 3.6e-6 + 1.8e-7 = 3.8e-6.
  * T leg: T_next is the product of one (1 - alpha) factor per composited entry, each with the subtraction's and the
    product's rounding (2 eps) plus its alpha's error scaled by alpha / (1 - alpha), which the clamp bounds by 999 but
    which a pixel near the stop threshold cannot collect often: n factors cost at most n (2 eps) + sum alpha-errors; the
    model takes (2 eps + 3.8e-6 / 4) per composited entry, i.e. 1.07e-6 n, and at least the alpha leg.
DELTA allows 4 x the model and is never above 1e-4 (IMAGE_RTOL, the project's own definition of sitting on a threshold):
delta_alpha = 1.5e-5; delta_T(n) = min(1e-4, max(1.5e-5, 4.3e-6 n)).  fp16-staged records are decoded before the walk, so
their rounding is in the records, not in the model.
"""
import numpy as np
import torch

from oracle.gsplat_oracle import ALPHA_MAX, ALPHA_MIN, ED_ALPHA_CLAMP

T_STOP = float(np.float32(1e-4))  # GSL_T_STOP as the kernels hold it
SEG_DEFAULT = 128
MUTANTS = ("stop_after", "last_is_stop", "skip32", "no_clamp", "pair_second", "rewalk_next_segment",
           "combine_last_segment", "cull98")
EPS32 = 2.0 ** -24
DELTA_ALPHA = 4.0 * (11 * EPS32 * 8.0 * np.log(2.0) + 3 * EPS32)
DELTA_T_PER_ENTRY = 4.0 * (2 * EPS32 + DELTA_ALPHA / 16.0)
DELTA_MAX = 1e-4


def delta_T(n_composited):
    """The T-leg of DELTA for a pixel that composited n entries (array or scalar)."""
    return np.minimum(DELTA_MAX, np.maximum(DELTA_ALPHA, DELTA_T_PER_ENTRY * np.asarray(n_composited, dtype=np.float64)))


def tile_pixels(tx, ty):
    """Centres of the 256 pixels of tile (tx, ty), row-major (pixel p = 16 row + column)."""
    j, i = np.meshgrid(np.arange(16), np.arange(16))
    return (16.0 * tx + j.reshape(-1) + 0.5), (16.0 * ty + i.reshape(-1) + 0.5)


def walk(rec, ids, px, py, active=None, dtype=np.float64, force=None, mutant=None, tile_xy=(0, 0), seg=SEG_DEFAULT,
         keep_below=None, track_slots=False):
    """The reference loop over the list `ids` (record rows, front to back) for the pixels (px, py).

    rec: dict of arrays over the Gaussians: x, y, a, b, c, op, feat [N, D] (and r, the cull radius, for three mutants).
    active: [P] bool, pixels that exist (inside the image and the pixel-row window); the others composite nothing.
    Returns a dict of per-pixel arrays: pix [P, D], T, last (list-relative, -1: none), stop (-1: none), n (entries
    composited), comp [P, L] bool, margin_alpha, margin_T, slot [P] (with track_slots, which reads the cull radius but
    changes no decision: was the stopping entry the first or the second candidate of the pair the kernel pops), and -- with
    keep_below=d -- near: a list of (kind, pixel, entry, margin) of every decision taken with a margin below d."""
    f = dtype
    px, py = np.asarray(px, dtype=f), np.asarray(py, dtype=f)
    P, L = px.shape[0], len(ids)
    D = rec["feat"].shape[1]
    done = np.zeros(P, dtype=bool) if active is None else ~np.asarray(active, dtype=bool)
    T = np.ones(P, dtype=f)
    pix = np.zeros((P, D), dtype=f)
    last = np.full(P, -1, dtype=np.int64)
    stop_at = np.full(P, -1, dtype=np.int64)
    stop_slot = np.full(P, -1, dtype=np.int64)
    ncomp = np.zeros(P, dtype=np.int64)
    comp = np.zeros((P, L), dtype=bool)
    m_alpha = np.full(P, np.inf)
    m_T = np.full(P, np.inf)
    near = []
    weights = np.zeros(L) if P == 1 else None  # alpha T of every entry a single pixel composited
    by_entry = {}
    for kind, p, k in (force or ()):
        by_entry.setdefault(int(k), []).append((kind, int(p)))
    amax, amin, tstop = f(ALPHA_MAX), f(ALPHA_MIN), f(T_STOP)
    geometric = track_slots or mutant in ("skip32", "pair_second", "cull98")
    if geometric:
        x0, y0 = 16.0 * tile_xy[0], 16.0 * tile_xy[1]
        quad = ((py - y0) >= 8).astype(np.int64) * 2 + ((px - x0) >= 8).astype(np.int64)  # wave = quadrant
        qcx, qcy = x0 + 4.0 + 8.0 * (np.arange(4) & 1), y0 + 4.0 + 8.0 * (np.arange(4) >> 1)
        cand_pos = np.zeros(4, dtype=np.int64)   # candidates of the quadrant in this batch of 256 records so far
        cnt = np.zeros(P, dtype=np.int64)        # candidates of the pixel's own mask in this half chunk so far
        pending = np.zeros(P, dtype=bool)        # pair_second: stopped on slot 0, slot 1 still to come
    stopped_in_seg = np.full(P, -1, dtype=np.int64)
    X, Y, A, B, C, O = (np.asarray(rec[k], dtype=f) for k in ("x", "y", "a", "b", "c", "op"))
    F = np.asarray(rec["feat"], dtype=f)
    for k, g in enumerate(np.asarray(ids, dtype=np.int64)):
        if mutant == "rewalk_next_segment" and k % seg == 0 and k > 0:
            again = stopped_in_seg == (k // seg - 1)  # stopped in the segment just ended: walked again here
            done &= ~again
        dx, dy = X[g] - px, Y[g] - py
        sigma = f(0.5) * (A[g] * dx * dx + C[g] * dy * dy) + B[g] * dx * dy
        raw = O[g] * np.exp(-sigma)
        alpha = raw if mutant == "no_clamp" else np.minimum(amax, raw)
        reach = ~done & (sigma >= 0)
        ok = alpha >= amin
        skip = np.zeros(P, dtype=bool)
        slot = np.zeros(P, dtype=np.int64)
        if geometric:
            r = float(rec["r"][g])
            if k % 256 == 0:
                cand_pos[:] = 0
            is_cand = (np.abs(X[g] - qcx) <= r + 3.5) & (np.abs(Y[g] - qcy) <= r + 3.5)
            pos = cand_pos.copy()
            cand_pos += is_cand
            new_half = (is_cand & (pos % 32 == 0))[quad]
            cnt[new_half] = 0
            pending &= ~new_half
            rr = 0.98 * r if mutant == "cull98" else r
            covers = is_cand[quad] & (np.abs(dx) <= rr) & (np.abs(dy) <= rr)
            slot = cnt % 2
            cnt += covers
            if mutant == "cull98":
                skip = ~covers
            if mutant == "skip32":
                skip = (pos % 64 == 32)[quad]
        with np.errstate(divide="ignore", invalid="ignore"):
            ma = np.abs(alpha / amin - 1.0)
        if k in by_entry:
            for kind, p in by_entry[k]:
                if kind == "alpha":
                    ok[p] = ~ok[p]
                    ma[p] = np.inf
        ok &= reach & ~skip
        m_alpha = np.where(reach, np.minimum(m_alpha, ma), m_alpha)
        Tn = T * (f(1.0) - alpha)
        stops = Tn <= tstop
        mt = np.abs(Tn / tstop - 1.0)
        if k in by_entry:
            for kind, p in by_entry[k]:
                if kind == "T":
                    stops[p] = ~stops[p]
                    mt[p] = np.inf
        m_T = np.where(ok, np.minimum(m_T, mt), m_T)
        if keep_below is not None:
            for p in np.nonzero(reach & (ma < keep_below))[0]:
                near.append(("alpha", int(p), k, float(ma[p])))
            for p in np.nonzero(ok & (mt < keep_below))[0]:
                near.append(("T", int(p), k, float(mt[p])))
        stop_now = ok & stops
        eff = ok & ~stops
        if mutant == "stop_after":
            eff = ok  # the stopping entry is composited, then the pixel stops
        if mutant == "pair_second":
            late = pending & (sigma >= 0) & (alpha >= amin) & ~stops & covers & (slot == 1)
            pending &= ~covers
            eff = eff | late
            pending |= stop_now & covers & (slot == 0)
        w = np.where(eff, alpha * T, f(0.0))
        pix += w[:, None] * F[g][None, :]
        if weights is not None:
            weights[k] = float(w[0])
        T = np.where(eff, Tn, T)
        last = np.where(eff, k, last)
        if mutant == "last_is_stop":
            last = np.where(stop_now, k, last)
        ncomp += eff
        comp[:, k] = eff
        stop_at = np.where(stop_now, k, stop_at)
        stop_slot = np.where(stop_now, slot, stop_slot)
        stopped_in_seg = np.where(stop_now, k // seg, stopped_in_seg)
        done = done | stop_now
    out = dict(pix=pix, T=T, last=last, stop=stop_at, n=ncomp, comp=comp, margin_alpha=m_alpha, margin_T=m_T,
               slot=stop_slot)
    if keep_below is not None:
        out["near"] = near
    if weights is not None:
        out["weights"] = weights
    return out


# ---------------------------------------------------------------------------------------------------------------------
# records
# ---------------------------------------------------------------------------------------------------------------------
def features_of(mode, depth, colours):
    """[N, D] features of a render mode: colours first, the depth feature last."""
    cols = []
    if mode.startswith("RGB"):
        cols.append(np.asarray(colours, dtype=np.float64)[:, :3])
    if mode != "RGB":
        cols.append(np.asarray(depth, dtype=np.float64)[:, None])
    return np.concatenate(cols, axis=1)


def _halves(words, high):
    """The low or high float16 of each int32 dword."""
    u = words.astype(np.int64) & 0xFFFFFFFF
    h = ((u >> 16) if high else (u & 0xFFFF)).astype(np.uint16)
    return h.view(np.float16).astype(np.float64)


def records_from_context(rc):
    """The records the compositing kernels of a RenderContext read after a forward, and its lists:
    (rec, offs [n_tiles + 1], flat [n]).  staging="fp16": decoded from rc.Qh by the dword layout of gsloc_common.h --
    dw0 x, dw1 y, dw2 (a | b), dw3 (c | r_cull), dw4 (0 | opacity), dw5 (r | g), dw6 (b | 0), dw7 depth.  With placement
    the lists index storage order, as the records do."""
    if rc.Qh is not None:
        q = rc.Qh.cpu().numpy().astype(np.int32)
        f32 = lambda col: np.ascontiguousarray(q[:, col]).view(np.float32).astype(np.float64)  # noqa: E731
        rec = dict(x=f32(0), y=f32(1), a=_halves(q[:, 2], False), b=_halves(q[:, 2], True), c=_halves(q[:, 3], False),
                   r=_halves(q[:, 3], True), op=_halves(q[:, 4], True))
        q0, q1 = rc.Q0.cpu().double().numpy(), rc.Q1.cpu().double().numpy()  # the float32 sources of the halves
        rec["src"] = dict(a=q1[:, 0], b=q1[:, 1], c=q1[:, 2], op=q0[:, 3])
        depth = f32(7)
        colours = np.stack([_halves(q[:, 5], False), _halves(q[:, 5], True), _halves(q[:, 6], False)], 1)
    else:
        q0, q1 = rc.Q0.cpu().double().numpy(), rc.Q1.cpu().double().numpy()
        rec = dict(x=q0[:, 0], y=q0[:, 1], op=q0[:, 3], a=q1[:, 0], b=q1[:, 1], c=q1[:, 2], r=q1[:, 3])
        depth = q0[:, 2]
        colours = rc.Q2.cpu().double().numpy()[:, :3] if rc.Q2 is not None else None
    rec["feat"] = features_of(rc.mode, depth, colours)
    n = min(int(rc.n_is.item()), rc.capacity)
    return rec, rc.offs.cpu().numpy().astype(np.int64), rc.flatten_ids[:n].cpu().numpy().astype(np.int64)


def cull_radius(a, b, c, op):
    """cull_radius of gsplatloc_amd/csrc/fused_project.hip in float64 (only the mutants read a radius)."""
    a, b, c, op = (np.asarray(t, dtype=np.float64) for t in (a, b, c, op))
    with np.errstate(divide="ignore", invalid="ignore"):
        tau = np.log(255.0 * op) * 1.01 + 0.01
        root = np.sqrt((0.5 * (a - c)) ** 2 + b * b)
        lmin = (a * c - b * b) / (0.5 * (a + c) + root)
        r = np.sqrt(2.0 * tau / lmin) * 1.0001 + 1e-3
    return np.where(tau > 0, r, -1.0)


def records_from_oracle(sc, mode, half=False):
    """The same records from the oracle's float32 projection of a scene (tests/stop_scenes.py), with the oracle's lists:
    what the CPU tests and the scene construction walk.  half=True rounds what an fp16-staged record holds."""
    from oracle import gsplat_oracle as G
    W, H = sc["W"], sc["H"]
    radii, m2, depths, conics, _ = G.fully_fused_projection(sc["means"], sc["quats"], sc["scales"], sc["V"][None],
                                                            sc["K"][None], W, H)
    tw, th = (W + 15) // 16, (H + 15) // 16
    _, isect_ids, flat = G.isect_tiles(m2, radii, depths, 16, tw, th)
    offs = G.isect_offset_encode(isect_ids, 1, tw, th).reshape(-1)
    h = (lambda t: t.half().double().numpy()) if half else (lambda t: t.double().numpy())
    con, op = h(conics[0]), h(sc["opacities"])
    rec = dict(x=m2[0, :, 0].double().numpy(), y=m2[0, :, 1].double().numpy(), a=con[:, 0], b=con[:, 1], c=con[:, 2], op=op)
    rec["r"] = cull_radius(conics[0, :, 0], conics[0, :, 1], conics[0, :, 2], sc["opacities"])
    rec["feat"] = features_of(mode, depths[0].double().numpy(), h(sc["rgb"]))
    offs = np.concatenate([offs.numpy().astype(np.int64), [flat.numel()]])
    return rec, offs, flat.numpy().astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# a frame, as the kernels write it
# ---------------------------------------------------------------------------------------------------------------------
def frame_reference(rec, offs, flat, W, H, ed, tile_rows=None, pixel_rows=None, long_min=0, seg=SEG_DEFAULT, mutant=None,
                    dtype=np.float64, force=None, keep_below=None, tiles=None):
    """The walk of every tile of the strip (`tiles`: only these).  Returns a dict: render [H, W, D], alphas [H, W, 1],
    T, last_ids, stop (list-relative), n, margin_alpha, margin_T [H, W], written [H, W] bool (pixels the forward
    writes), hits {(tile, quadrant): uint32 words} for the tiles that are not split, per_tile {tile: walk result}.
    force: {tile: [(kind, pixel, entry), ...]}."""
    tw, th = (W + 15) // 16, (H + 15) // 16
    ty0, ty1 = tile_rows if tile_rows is not None else (0, th)
    row0, row1 = pixel_rows if pixel_rows is not None else (ty0 * 16, min(ty1 * 16, H))
    D = rec["feat"].shape[1]
    out = dict(render=np.zeros((H, W, D)), alphas=np.zeros((H, W, 1)), T=np.ones((H, W)),
               last_ids=np.zeros((H, W), dtype=np.int64), stop=np.full((H, W), -1, dtype=np.int64),
               n=np.zeros((H, W), dtype=np.int64), margin_alpha=np.full((H, W), np.inf),
               margin_T=np.full((H, W), np.inf), written=np.zeros((H, W), dtype=bool), hits={}, per_tile={})
    for ty in range(ty0, ty1):
        for tx in range(tw):
            t = ty * tw + tx
            if tiles is not None and t not in tiles:
                continue
            rs, re = int(offs[t]), int(offs[t + 1])
            px, py = tile_pixels(tx, ty)
            ii, jj = (py - 0.5).astype(np.int64), (px - 0.5).astype(np.int64)
            act = (ii < H) & (jj < W) & (ii >= row0) & (ii < row1)
            is_long = long_min > 0 and re - rs > long_min
            res = walk(rec, flat[rs:re], px, py, act, dtype=dtype, mutant=mutant, tile_xy=(tx, ty), seg=seg,
                       force=(force or {}).get(t), keep_below=keep_below)
            out["per_tile"][t] = res
            last = res["last"].copy()
            if mutant == "combine_last_segment" and is_long:
                # the combine takes the last index of the last segment it visited, even when that composited nothing
                visited = np.where(res["stop"] >= 0, res["stop"], re - rs - 1) // seg
                last = np.where(last // seg == visited, last, -1)
            A = 1.0 - res["T"]
            pix = res["pix"].astype(np.float64).copy()
            if ed:
                pix[:, -1] = pix[:, -1] / np.maximum(A, ED_ALPHA_CLAMP)
            i_a, j_a = ii[act], jj[act]
            out["render"][i_a, j_a] = pix[act]
            out["alphas"][i_a, j_a, 0] = A[act]
            out["T"][i_a, j_a] = res["T"][act]
            out["last_ids"][i_a, j_a] = np.where(last >= 0, rs + last, 0)[act]
            out["written"][i_a, j_a] = True
            for key in ("stop", "n", "margin_alpha", "margin_T"):
                out[key][i_a, j_a] = res[key][act]
            if not is_long:
                li, lj = ii - 16 * ty, jj - 16 * tx
                quad = (li >= 8) * 2 + (lj >= 8)
                block = ((li & 7) >= 4) * 2 + ((lj & 7) >= 4)
                for q in range(4):
                    nib = np.zeros(re - rs, dtype=np.uint32)
                    for b in range(4):
                        sel = (quad == q) & (block == b)
                        nib |= (res["comp"][sel].any(0).astype(np.uint32) << b)
                    k = np.nonzero(nib)[0]
                    out["hits"][(t, q)] = (nib[k] << np.uint32(28)) | (rs + k).astype(np.uint32)
    return out


def context_hits(rc, offs):
    """{(tile, quadrant): uint32 words} of the hit lists a forward of the context wrote."""
    counts = rc.hit_counts.cpu().numpy()
    words = rc.hits.cpu().numpy().view(np.uint32)
    out = {}
    for t in range(rc.ty0 * rc.tw, rc.ty1 * rc.tw):
        rs, re = int(offs[t]), int(offs[t + 1])
        for q in range(4):
            a = 4 * rs + q * (re - rs)
            out[(t, q)] = words[a:a + int(counts[4 * t + q])].copy()
    return out


def compare_frames(got, ref, rtol, atol, hits=True):
    """Every pixel, no allowance: render and alphas within atol + rtol |ref|, last_ids equal, pixels the forward does
    not write untouched (`got["untouched"]`: bool [H, W], if given), hit lists equal word for word on the tiles the
    reference has them for.  Returns (failures: list of str, figures: dict of the largest errors)."""
    fails, figs = [], {}
    w = ref["written"]
    for key in ("render", "alphas"):
        g, r = np.asarray(got[key], dtype=np.float64), ref[key]
        err = np.abs(g - r)
        bad = (err > atol + rtol * np.abs(r)).any(-1) & w
        figs[key] = float((err / (atol + rtol * np.abs(r)))[w].max()) if w.any() else 0.0  # in units of the tolerance
        if bad.any():
            i, j = np.argwhere(bad)[0]
            fails.append(f"{key}: {int(bad.sum())} pixels outside the tolerance, first ({i}, {j}): {g[i, j]} vs {r[i, j]}")
    gl = np.asarray(got["last_ids"], dtype=np.int64)
    bad = (gl != ref["last_ids"]) & w
    if bad.any():
        i, j = np.argwhere(bad)[0]
        fails.append(f"last_ids: {int(bad.sum())} pixels differ, first ({i}, {j}): {gl[i, j]} vs {ref['last_ids'][i, j]}")
    if got.get("untouched") is not None and not np.asarray(got["untouched"])[~w].all():
        fails.append("a pixel outside the image or the pixel-row window was written")
    if hits and got.get("hits") is not None:
        for key, want in ref["hits"].items():
            have = got["hits"].get(key)
            if have is None or have.shape != want.shape or (have != want).any():
                fails.append(f"hit list of tile {key[0]} quadrant {key[1]}: {None if have is None else have.shape[0]} "
                             f"words vs {want.shape[0]}, or other words")
                break
    return fails, figs


HALF_FIELDS = ("a", "b", "c", "op")


def _half_neighbour(h, up):
    """The float16 next to h (a float holding a half), upwards or downwards."""
    return float(np.nextafter(np.float16(h), np.float16(np.inf if up else -np.inf)))


def _rounding_candidates(rec, ids, comp_entries, rgb, weights):
    """Half entries of the records a pixel composited that could have been rounded the other way: for the conic and the
    opacity, whose float32 sources the context keeps (rec["src"]), those whose source lies within DELTA_MAX (relative) of
    the midpoint between two halves, nearest first, six at most; then the colours (read from the half record only),
    either way, of the entries heavy enough for half an ulp of a half (4.9e-4) to show at the tolerance (alpha T >= 0.02)."""
    out = []
    for k in comp_entries:
        g = int(ids[k])
        for f in HALF_FIELDS:
            v, h = float(rec["src"][f][g]), float(rec[f][g])
            nb = _half_neighbour(h, v > h) if v != h else None
            if nb is None or v == 0.0:
                continue
            m = abs(v - 0.5 * (h + nb)) / abs(v)
            if m < DELTA_MAX:
                out.append((m, f, g, nb))
    out.sort()
    out = out[:6]
    if rgb:
        for k in comp_entries:
            g = int(ids[k])
            if weights[k] < 0.02:
                continue
            for ch in range(3):
                for up in (False, True):
                    out.append((np.inf, ("feat", ch), g, _half_neighbour(float(rec["feat"][g, ch]), up)))
    return out


def _with_rounding(rec, flips):
    r = dict(rec)
    for _m, f, g, nb in flips:
        key, ch = (f, None) if isinstance(f, str) else f
        r[key] = np.array(r[key], dtype=np.float64, copy=True)
        if ch is None:
            r[key][g] = nb
        else:
            r[key][g, ch] = nb
    return r


def explain_pixels(rec, offs, flat, W, H, ed, got, suspects, tile_rows=None, pixel_rows=None, rtol=1e-4, atol=2e-5,
                   max_forced=2, oracle=None, rgb=False):
    """Every pixel where `got` (render, alphas, last_ids of a kernel) differs from the walk, and every pixel of
    `suspects` ([H, W] bool: what a comparison with the end-to-end oracle rejected), must sit on a threshold:

      * the walk reports a decision with a margin below DELTA for it, and the kernel's pixel equals the walk with at
        most `max_forced` of those decisions forced the other way (render, alpha and last index); or
      * for a pixel where the kernel AGREES with the walk of its own records (so nothing the compositing kernel did is in
        question) and no decision is below the kernel's DELTA: the oracle projects in float64, the records are the float32
        projection -- at a camera far from the origin that alone moves alpha by several 1e-5 (tests/parity.py) -- so the
        decision may sit up to the cap DELTA_MAX = 1e-4 from its threshold, and then the ORACLE's pixel (`oracle`: render,
        alphas) must equal the walk with at most `max_forced` of those decisions forced the other way; or
      * fp16-staged records only (rec["src"]: the float32 sources of the halves), for a pixel where the kernel AGREES with
        the walk of its own records: a half entry of a record the pixel composited sits on a float16 rounding boundary --
        the oracle rounds the float64 projection, the kernel the float32 one -- and the ORACLE's pixel (`oracle`: render,
        alphas) equals the walk with at most `max_forced` such entries rounded the other way.  (A finding of this test:
        in the fp16 cases of the ladder scenes every rejected pixel is of this kind, whole splats of them.)

    Returns (n_differ, n_explained, messages): pixels where the kernel differs from the walk, pixels explained, and one
    message per unexplained pixel (pixel, tile, quadrant, nearest decision)."""
    import itertools
    tw = (W + 15) // 16
    ref = frame_reference(rec, offs, flat, W, H, ed, tile_rows, pixel_rows)
    g_r, g_a = np.asarray(got["render"], dtype=np.float64), np.asarray(got["alphas"], dtype=np.float64).reshape(H, W)
    g_l = np.asarray(got["last_ids"], dtype=np.int64)

    def outputs(res):
        A = 1.0 - float(res["T"][0])
        pix = np.array(res["pix"][0], dtype=np.float64)
        if ed:
            pix[-1] = pix[-1] / max(A, ED_ALPHA_CLAMP)
        return pix, A

    def close(pix, A, t_pix, t_A, mine_is_reference=True):
        rp, ra = (pix, A) if mine_is_reference else (t_pix, t_A)
        return bool((np.abs(t_pix - pix) <= atol + rtol * np.abs(rp)).all() and abs(t_A - A) <= atol + rtol * abs(ra))

    mism = ((np.abs(g_r - ref["render"]) > atol + rtol * np.abs(ref["render"])).any(-1)
            | (np.abs(g_a - ref["alphas"][..., 0]) > atol + rtol * np.abs(ref["alphas"][..., 0]))
            | (g_l != ref["last_ids"])) & ref["written"]
    todo = mism | (np.asarray(suspects, dtype=bool) & ref["written"])
    explained, messages, winners = 0, [], []
    for i, j in np.argwhere(todo):
        tx, ty = int(j) // 16, int(i) // 16
        t = ty * tw + tx
        rs, re = int(offs[t]), int(offs[t + 1])
        ids = flat[rs:re]
        one = (np.array([j + 0.5]), np.array([i + 0.5]))
        res = walk(rec, ids, *one, keep_below=DELTA_MAX)
        lim_T = float(delta_T(int(res["n"][0]) + 1))
        near = sorted((d for d in res["near"] if d[3] < (DELTA_ALPHA if d[0] == "alpha" else lim_T)), key=lambda d: d[3])
        where = f"pixel ({i}, {j}) tile ({tx}, {ty}) quadrant {(i % 16 >= 8) * 2 + (j % 16 >= 8)}"
        nearest = min(float(res["margin_alpha"][0]), float(res["margin_T"][0]))
        found = bool(near) and not mism[i, j]  # rejected by the oracle only: the kernel agrees with the walk, on a threshold
        for n_f in range(1, max_forced + 1) if (near and not found) else ():
            for combo in itertools.combinations(near[:6], n_f):
                f = walk(rec, ids, *one, force=[(kind, 0, k) for kind, _p, k, _m in combo])
                last = int(f["last"][0])
                if close(*outputs(f), g_r[i, j], g_a[i, j]) and g_l[i, j] == (rs + last if last >= 0 else 0):
                    found = True
                    break
            if found:
                break
        if not found and not mism[i, j] and oracle is not None:
            o_pix, o_A = np.asarray(oracle[0], dtype=np.float64)[i, j], float(np.asarray(oracle[1], dtype=np.float64).reshape(H, W)[i, j])
            capped = sorted(res["near"], key=lambda d: d[3])[:6]  # every decision below the cap DELTA_MAX, nearest first
            for combo in (c for n_f in range(1, max_forced + 1) for c in itertools.combinations(capped, n_f)):
                f = walk(rec, ids, *one, force=[(kind, 0, k) for kind, _p, k, _m in combo])
                if close(*outputs(f), o_pix, o_A, mine_is_reference=False):
                    found = True
                    break
        if not found and not mism[i, j] and "src" in rec and oracle is not None:
            entries = np.nonzero(res["comp"][0])[0].tolist() + ([int(res["stop"][0])] if res["stop"][0] >= 0 else [])
            cands = _rounding_candidates(rec, ids, entries, rgb, res["weights"])
            sourced = [c for c in cands if c[0] < np.inf]
            in_list = set(int(x) for x in ids[entries])
            trials = [(w,) for w in winners if w[2] in in_list] + [(c,) for c in cands]
            trials += list(itertools.combinations(sourced[:6], 2)) if max_forced >= 2 else []
            for flips in trials:
                f = walk(_with_rounding(rec, flips), ids, *one)
                if close(*outputs(f), o_pix, o_A, mine_is_reference=False):
                    found = True
                    winners += [c for c in flips if c not in winners]
                    break
        if found:
            explained += 1
        elif not near:
            messages.append(f"{where}: {'differs from the walk, ' if mism[i, j] else ''}no decision below DELTA (nearest "
                            f"margin {nearest:.2e}, {int(res['n'][0])} entries composited)")
        else:
            messages.append(f"{where}: differs from the walk and no {max_forced} of its {len(near)} near-threshold "
                            f"decisions explain it (nearest margin {nearest:.2e})")
    return int(mism.sum()), explained, messages


def assert_flips_explained(tag, rc, render, alphas, suspects, oracle=None):
    """The assertion of the random-scene tests: every pixel of a RenderContext's forward that `suspects` marks (rejected
    against the end-to-end oracle, whose render and alphas are `oracle`) or that differs from the walk of the context's
    own records sits on a threshold and is explained by it (explain_pixels).  Prints the counts before it asserts."""
    rec, offs, flat = records_from_context(rc)
    got = to_numpy_frame(render, alphas, rc.last_ids)
    sus = np.asarray(torch.as_tensor(suspects).cpu().numpy(), dtype=bool).reshape(rc.H, rc.W)
    if oracle is not None:
        oracle = tuple(torch.as_tensor(t).detach().cpu().double().numpy() for t in oracle)
    n_differ, explained, messages = explain_pixels(rec, offs, flat, rc.W, rc.H, rc.ed, got, sus, (rc.ty0, rc.ty1),
                                                   (rc.row0, rc.row1), oracle=oracle, rgb=rc.rgb)
    print(f"[explained] {tag}: {int(sus.sum())} pixels rejected against the oracle, {n_differ} differ from the walk of the "
          f"records, {explained} explained, {len(messages)} unexplained")
    assert not messages, (tag, "unexplained pixels", messages[:8])
    return explained


def to_numpy_frame(render, alphas, last_ids):
    return dict(render=torch.as_tensor(render).detach().cpu().double().numpy(),
                alphas=torch.as_tensor(alphas).detach().cpu().double().numpy().reshape(render.shape[0], render.shape[1], 1),
                last_ids=torch.as_tensor(last_ids).detach().cpu().numpy().astype(np.int64))
