"""The record-level walk (tests/walk_ref.py) and the stop-ladder scenes (tests/stop_scenes.py), without a GPU:

  * the walker equals the oracle's rasterize_to_pixels in float64 on the same records (the two references are one);
  * the scene condition holds: no decision of any pixel within CPU_MARGIN of a threshold, on the plain and on the
    half-rounded records of the float32 oracle projection;
  * every case the scenes are built for is really present: list lengths, the stopping index of a pixel per target, the
    spread of stopping indices within a quadrant, both slots of a pair, candidate position = list position;
  * the comparator of tests/test_gpu_fwd_decisions.py has teeth: each of eight deliberately wrong walks is rejected on at
    least one scene, and the float32 run of the correct walk is not;
  * on the random scenes of tests/test_gpu_grad_paths.py at most 1 % of the pixels have a decision below the explanation
    threshold DELTA (measured: none, 0.004 % and 0.007 %), so "explained by a threshold" cannot excuse a defect of a quadrant.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import gsplat_oracle as G
from tests import stop_scenes as S
from tests import walk_ref as WR
from tests.parity import IMAGE_ATOL, IMAGE_RTOL

LONG_MIN = 2048  # gsplatloc_amd.context.LONG_MIN (asserted on the GPU, where the package loads its library)


@functools.lru_cache(maxsize=None)
def _frame(name, half=False, mutant=None, dtype="f64"):
    sc = S.scene(name)
    rec, offs, flat = WR.records_from_oracle(sc, "RGB+ED", half)
    ref = WR.frame_reference(rec, offs, flat, sc["W"], sc["H"], True, long_min=LONG_MIN if name in S.LONG_SCENES else 0,
                             mutant=mutant, dtype=np.float64 if dtype == "f64" else np.float32)
    return sc, rec, offs, flat, ref


def _tile(sc, t):
    return t[1] * ((sc["W"] + 15) // 16) + t[0]


@pytest.mark.parametrize("name", ["short", "ragged", "long-b"])
def test_the_walker_equals_the_oracle_compositing_in_float64(name):
    sc, rec, offs, flat, ref = _frame(name)
    W, H = sc["W"], sc["H"]
    tw, th = (W + 15) // 16, (H + 15) // 16
    t = lambda k: torch.from_numpy(np.asarray(rec[k], dtype=np.float64))  # noqa: E731
    rc, ra = G.rasterize_to_pixels(torch.stack([t("x"), t("y")], -1)[None], torch.stack([t("a"), t("b"), t("c")], -1)[None],
                                   t("feat")[None], t("op")[None], W, H, 16,
                                   torch.from_numpy(offs[:-1]).reshape(1, th, tw), torch.from_numpy(flat))
    rc = torch.cat([rc[..., :-1], rc[..., -1:] / ra.clamp(min=G.ED_ALPHA_CLAMP)], -1)
    assert np.abs(rc[0].numpy() - ref["render"]).max() < 1e-12
    assert np.abs(ra[0].numpy() - ref["alphas"]).max() < 1e-13
    assert float(ra.max()) > 0.99 and int((ref["stop"] >= 0).sum()) > 0


@pytest.mark.parametrize("half", [False, True], ids=["fp32-records", "fp16-records"])
@pytest.mark.parametrize("name", list(S.SCENES))
def test_no_decision_of_any_pixel_is_near_a_threshold(name, half):
    sc, rec, offs, flat, ref = _frame(name, half)
    worst = min(float(ref["margin_alpha"].min()), float(ref["margin_T"].min()))
    print(f"[scene] {name} half={half}: smallest margin alpha {ref['margin_alpha'].min():.2e}, T {ref['margin_T'].min():.2e}; "
          f"{sc['nudged']} nudges of 1 %")
    assert worst >= S.CPU_MARGIN, f"scene too close to a threshold: {name} half={half} {worst:.2e}"
    # the float32 walk takes every decision as the float64 walk does
    ref32 = _frame(name, half, None, "f32")[4]
    assert (ref32["last_ids"] == ref["last_ids"]).all() and (ref32["stop"] == ref["stop"]).all()


@pytest.mark.parametrize("name", list(S.SCENES))
def test_every_required_case_is_present(name):
    sc, rec, offs, flat, ref = _frame(name)
    slots = set()
    for t, spec in sc["tiles"].items():
        ti = _tile(sc, t)
        res = ref["per_tile"][ti]
        rs, re = int(offs[ti]), int(offs[ti + 1])
        assert re - rs == spec["n"], (name, t, re - rs)
        x0, y0 = 16 * t[0], 16 * t[1]
        stops = res["stop"]
        # every entry that matters is a candidate of all four quadrants: candidate position = list position in the batch
        ids = flat[rs:re]
        real = rec["op"][ids] > 1.0 / 255.0
        for q in range(4):
            cx, cy = x0 + 4.0 + 8.0 * (q & 1), y0 + 4.0 + 8.0 * (q >> 1)
            cand = (np.abs(rec["x"][ids] - cx) <= rec["r"][ids] + 3.5) & (np.abs(rec["y"][ids] - cy) <= rec["r"][ids] + 3.5)
            if not spec.get("compact") and not any(k in spec for k in ("early", "faint", "dots")):
                assert cand[real].all(), (name, t, q)
            assert not cand[~real].any(), (name, t, q, "a ghost is a candidate")
        for tg in spec.get("targets", ()):
            p = tg["pixel"][1] * 16 + tg["pixel"][0]
            assert stops[p] == tg["p"], (name, t, tg, int(stops[p]))
            assert res["last"][p] < tg["p"] and res["comp"][p, tg["first"]] and not res["comp"][p, tg["p"]]
            assert abs(res["T"][p] / WR.T_STOP - 1.0) > 0.5  # T is the value BEFORE the stop, well above 1e-4
        if spec.get("targets"):
            px, py = WR.tile_pixels(*t)
            slotted = WR.walk(rec, ids, px, py, tile_xy=t, track_slots=True)
            assert (slotted["stop"] == stops).all() and (slotted["last"] == res["last"]).all()
            slots |= set(slotted["slot"][stops >= 0].tolist())
        if "strong" in spec:
            s, c = spec["strong"]
            li, lj = np.arange(256) // 16, np.arange(256) % 16
            quad = (li >= 8) * 2 + (lj >= 8)
            spread = [len(set(stops[(quad == q) & (stops >= 0)].tolist())) for q in range(4)]
            assert max(spread) >= (2 if spec.get("compact") else 3), (name, t, spread)
            hit = stops[stops >= 0]
            assert hit.min() >= s and hit.max() < s + c + 8, (name, t, int(hit.min()), int(hit.max()))
            seam = {(0, 2): None, (1, 2): 64, (2, 2): 256 if name == "short" else 128, (0, 1): 1280}.get(t)
            if seam is not None and name in ("short", "long-c"):
                assert hit.min() < seam <= hit.max(), (name, t, "the run does not stop pixels on both sides of", seam)
        if not spec.get("targets") and "strong" not in spec and not spec.get("dots"):
            assert (stops < 0).all(), (name, t, "a list that never stops")
        if spec.get("faint"):
            act = res["n"] > 0
            assert int(act.sum()) == 1 and 0.0 < float(1.0 - res["T"][act][0]) < 1.1 / 255.0
        if "early" in spec:
            k, (i, j) = spec["early"]
            p = j * 16 + i
            assert res["last"][p] == k and res["n"][p] == 1 and stops[p] < 0 and spec["n"] > LONG_MIN
    if name == "short":
        t = _tile(sc, (0, 0))
        p = 8 * 16 + 8
        assert ref["per_tile"][t]["stop"][p] == 1 and ref["per_tile"][t]["last"][p] == 0  # the second of two 0.999 entries
        assert slots >= {0, 1}, "stops on the first and on the second candidate of a pair"
        assert sc["tiles"][(1, 1)]["n"] % 2 == 1 and (2, 1) not in sc["tiles"]
        t = _tile(sc, (2, 1))
        assert offs[t + 1] == offs[t] and not ref["alphas"][16:32, 32:48].any()  # the blank tile
        want = {1, 30, 31, 32, 33, 62, 63, 64, 65, 127, 128, 255, 256, 257, 299}
        have = set(ref["stop"][ref["stop"] >= 0].tolist())
        assert want <= have, sorted(want - have)
    if name == "ragged":
        assert sc["W"] % 16 == 8 and sc["H"] % 16 == 8 and int((ref["stop"][32:, 48:] >= 0).sum()) == 1  # the corner tile
    if name in S.LONG_SCENES:
        seg = WR.SEG_DEFAULT
        have = set(ref["stop"][ref["stop"] >= 0].tolist())
        want = {"long-a": {5, 383, 384, 385, 767, 768, 1023, 1024}, "long-b": {639, 640, 1920, 2176}, "long-c": {1279, 1280}}[name]
        assert want <= have, (name, sorted(want - have))
        for t, spec in sc["tiles"].items():
            if spec["n"] > LONG_MIN:
                nseg = -(-spec["n"] // seg)
                assert 2049 <= spec["n"] <= 2700 and nseg > 8
    if name == "long-a":  # 3 x 128 +- 1 inside a quarter; 6 x 128 is the first quarter seam of 21 segments; segments 7 | 8
        assert -(-2600 // 128) == 21 and -(-21 // 4) == 6
    if name == "long-b":  # 2177 = 17 x 128 + 1: the last entry is a segment of its own; 18 segments, quarters of 5
        assert -(-2177 // 128) == 18 and 639 == 5 * 128 - 1 and 1920 == 15 * 128


@pytest.mark.parametrize("mutant", WR.MUTANTS)
def test_the_comparator_rejects_the_mutant(mutant):
    """The comparator of the GPU test, on the mutated walk against the reference, fails on at least one scene."""
    rejected = []
    segmented = mutant in ("rewalk_next_segment", "combine_last_segment")  # defects of the split: long scenes only
    for name in S.LONG_SCENES if segmented else ("short", "long-a", "long-b", "long-c"):
        ref = _frame(name)[4]
        bad = _frame(name, False, mutant)[4]
        fails, _ = WR.compare_frames(bad, ref, IMAGE_RTOL, IMAGE_ATOL)
        if fails:
            rejected.append((name, fails[0]))
            break
    print(f"[mutant] {mutant}: {rejected}")
    assert rejected, f"no scene rejects the mutant {mutant}"


@pytest.mark.parametrize("name", list(S.SCENES))
def test_the_comparator_accepts_the_float32_walk(name):
    ref = _frame(name)[4]
    f32 = _frame(name, False, None, "f32")[4]
    fails, figs = WR.compare_frames(f32, ref, IMAGE_RTOL, IMAGE_ATOL)
    rel_T = float(np.abs(f32["T"].astype(np.float64) / ref["T"] - 1.0).max())
    print(f"[float32 walk] {name}: largest error / tolerance {figs}, t_final relative {rel_T:.2e}")
    assert not fails, fails
    assert rel_T < 2.5e-5  # (4 x this is the GPU test's t_final bound, itself capped at 1e-4)


@pytest.mark.parametrize("variant", ["ladder", "tiny", "long"])
def test_few_pixels_of_the_random_scenes_sit_below_the_explanation_threshold(variant):
    from tests.test_gpu_grad_paths import H, W, _ladder_scene
    sc = dict(_ladder_scene(variant))
    sc.update(W=W, H=H)
    rec, offs, flat = WR.records_from_oracle(sc, "RGB+ED")
    ref = WR.frame_reference(rec, offs, flat, W, H, True)
    below = (ref["margin_alpha"] < WR.DELTA_ALPHA) | (ref["margin_T"] < WR.delta_T(ref["n"] + 1))
    share = float(below.mean())
    print(f"[explanation threshold] {variant}: {share:.2e} of the pixels have a decision below DELTA")
    assert share <= 1e-2, (variant, share)


# ---------------------------------------------------------------------------------------------------------------------
# the explanation of flipped pixels (explain_pixels: the assertion added to the random-scene GPU tests)
# ---------------------------------------------------------------------------------------------------------------------
def _differs(a, b):
    return ((np.abs(a["render"] - b["render"]) > IMAGE_ATOL + IMAGE_RTOL * np.abs(b["render"])).any(-1)
            | (np.abs(a["alphas"] - b["alphas"])[..., 0] > IMAGE_ATOL + IMAGE_RTOL * np.abs(b["alphas"][..., 0])))


def test_a_defect_is_not_explained_by_a_threshold():
    """A frame of a mutated walk differs on dozens of pixels; none of them sits on a threshold, none is explained."""
    sc, rec, offs, flat, ref = _frame("short")
    none = np.zeros((sc["H"], sc["W"]), dtype=bool)
    assert WR.explain_pixels(rec, offs, flat, sc["W"], sc["H"], True, ref, none) == (0, 0, [])
    for mutant in ("stop_after", "cull98"):
        bad = _frame("short", False, mutant)[4]
        n, explained, messages = WR.explain_pixels(rec, offs, flat, sc["W"], sc["H"], True, bad, none)
        assert n >= 20 and explained == 0 and len(messages) == n, (mutant, n, explained)
        assert "tile (" in messages[0] and "quadrant" in messages[0] and "margin" in messages[0]


def test_a_forced_threshold_decision_is_explained():
    """On the random ladder scene, a "kernel" that takes one decision below DELTA the other way differs from the walk on
    that pixel and is explained; the same flip of a decision far from its threshold is not."""
    from tests.test_gpu_grad_paths import H, W, _ladder_scene
    sc = dict(_ladder_scene("long"))
    sc.update(W=W, H=H)
    rec, offs, flat = WR.records_from_oracle(sc, "RGB+ED")
    ref = WR.frame_reference(rec, offs, flat, W, H, True, keep_below=WR.DELTA_MAX)
    tw, none, tried = (W + 15) // 16, np.zeros((H, W), dtype=bool), 0

    def kernel_with(t, flip):
        forced = WR.frame_reference(rec, offs, flat, W, H, True, tiles={t}, force={t: [flip]})
        frame = {k: ref[k].copy() for k in ("render", "alphas", "last_ids")}
        ty, tx = divmod(t, tw)
        for k in frame:
            frame[k][16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16] = forced[k][16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16]
        return frame

    for t, res in ref["per_tile"].items():
        for kind, p, k, m in res["near"]:
            if m < (WR.DELTA_ALPHA if kind == "alpha" else float(WR.delta_T(res["n"][p] + 1))):
                assert WR.explain_pixels(rec, offs, flat, W, H, True, kernel_with(t, (kind, p, k)), none) == (1, 1, [])
                tried += 1
    assert tried >= 2
    t = 2 * tw + 4  # the 64-entry tile: its first entry, at the pixel it covers best
    res = ref["per_tile"][t]
    p = int(np.argmax(res["comp"][:, 0]))
    assert res["comp"][p, 0] and res["margin_alpha"][p] > 1e-3
    n, explained, messages = WR.explain_pixels(rec, offs, flat, W, H, True, kernel_with(t, ("alpha", p, 0)), none)
    assert (n, explained, len(messages)) == (1, 0, 1), (n, explained, messages)


def test_a_half_rounded_the_other_way_is_explained_and_a_defect_is_not():
    """fp16 records: the oracle rounds one conic entry of a stopper to the neighbouring half (its float32 source sits on
    the rounding boundary); the 29 pixels it rejects are explained.  An oracle that differs by a defect is not."""
    sc = S.scene("short")
    rec, offs, flat = WR.records_from_oracle(sc, "RGB+ED", half=True)
    full = WR.records_from_oracle(sc, "RGB+ED", half=False)[0]
    rec["src"] = {k: full[k].copy() for k in WR.HALF_FIELDS}
    ref = WR.frame_reference(rec, offs, flat, sc["W"], sc["H"], True)
    g = int(flat[offs[_tile(sc, (1, 2))] + 60])
    nb = WR._half_neighbour(rec["a"][g], True)
    rec["src"]["a"][g] = 0.5 * (rec["a"][g] + nb) * (1 - 1e-6)
    orc = WR.frame_reference(WR._with_rounding(rec, [(0.0, "a", g, nb)]), offs, flat, sc["W"], sc["H"], True)
    sus = _differs(ref, orc)
    assert int(sus.sum()) >= 20
    n, explained, messages = WR.explain_pixels(rec, offs, flat, sc["W"], sc["H"], True, ref, sus,
                                               oracle=(orc["render"], orc["alphas"]), rgb=True)
    assert (n, explained, messages) == (0, int(sus.sum()), [])
    bad = WR.frame_reference(rec, offs, flat, sc["W"], sc["H"], True, mutant="stop_after")
    sus = _differs(ref, bad)
    n, explained, messages = WR.explain_pixels(rec, offs, flat, sc["W"], sc["H"], True, ref, sus,
                                               oracle=(bad["render"], bad["alphas"]), rgb=True)
    # (a colour half next door can close a difference that is barely outside the tolerance: a few pixels, never all)
    assert n == 0 and len(messages) >= 20 and explained <= int(sus.sum()) // 8, (n, explained, int(sus.sum()))
