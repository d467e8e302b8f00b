"""The lens mode's restatement (tests/denoise_lens_reference.py) without a GPU: with cocK = 0 it is the two existing restatements bit for
bit; on a synthetic two-id image with a depth step the rule does what DESIGN.md section 3.5 says (a relaxed tap crosses the id edge, the
minimum of the two radii keeps a sharp side untouched, a NaN t relaxes nothing, a miss tap uses c = cocK); the host's cocK; and passes
that each break one part of the rule differ from the restatement on the recipes of tests/denoise_inputs.py."""
import numpy as np
import pytest

import denoise_input_cases as dc
import denoise_inputs as di
import denoise_lens_reference as dl
import denoise_reference as dr
import denoise_variance_reference as dv
import test_denoise_inputs_cpu as ti

F = np.float32
R = di.Recipe
same = dc.same


# ------------------------------------------------------------------------------------------------ 1. cocK = 0 is today's filter
@pytest.mark.parametrize("variance", [False, True], ids=["fixed", "variance"])
@pytest.mark.parametrize("shape", [(131, 67), (65, 17), (1, 40)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_without_a_blur_radius_the_passes_are_the_existing_restatements(shape, variance):
    g = ti.guides_for(shape)
    for recipe in (di.NOISE, R("finite_specials", True), R("subnormal_block", True), R("nonfinite_seed")):
        img = di.build(g["id"], recipe, 5)
        p = dr.Params(iterations=3)
        stats = dl.new_stats()
        got, got_v0 = dl.denoise(img, g, p, 6.0 if variance else None, 0.0, 20.0, stats=stats)
        want, want_v0 = dv.denoise(img, g, p, 6.0) if variance else (dr.denoise(img, g, p), None)
        assert (dc.bits(got) == dc.bits(want)).all(), recipe.name
        if variance:
            assert (dc.bits(got_v0) == dc.bits(want_v0)).all(), recipe.name
        assert stats["relaxed"] == 0 and stats["taps"] > 0


# ------------------------------------------------------------------------------------------------ 2. the rule on a depth step
H, W, SPLIT = 20, 40, 20


def step_guides(t_left=10.0, t_right=40.0, miss=False):
    """A head-on plane (pos = (x, y, 0) / 10, N = +z: w_n = w_z = 1 on every tap, so a relaxed tap weighs what an unrelaxed one of the
    same id does and only the taps that cross an id can change the result): id 0 at t_left left of column SPLIT, id 256 at t_right right
    of it; miss: the last four columns are misses."""
    ids = np.zeros((H, W), np.int32)
    ids[:, SPLIT:] = 256
    if miss:
        ids[:, W - 4:] = -1
    g = ti.plane_guides(ids)
    hit = ids >= 0
    g["t"] = np.where(hit, np.where(ids == 0, F(t_left), F(t_right)), F(np.inf))
    return g


def two_tone(g):
    img = np.ones((H, W, 4), F)
    img[..., :3] = np.where((g["id"] == 0)[..., None], F(0.25), F(0.5))  # (powers of two: a weighted mean of equal tones is exact)
    return img


WIDE = dr.Params(iterations=1, sigma_color=100.0)  # (a luminance stop that lets the two tones mix)


def test_a_relaxed_tap_crosses_the_id_edge():
    g = step_guides()  # F = 20, cocK = 4: c = 4 on the left (|10 - 20| / 10), 2 on the right (|40 - 20| / 40)
    c = dl.coc_radius(g, 4.0, 20.0)
    assert (c[:, :SPLIT] == 4).all() and (c[:, SPLIT:] == 2).all()
    img = two_tone(g)
    stats = dl.new_stats()
    out, _ = dl.denoise(img, g, WIDE, None, 4.0, 20.0, stats=stats)
    plain = dr.denoise(img, g, WIDE)
    assert stats["crossing"] > 0
    assert (plain[:, :SPLIT, 0] == F(0.25)).all() and (plain[:, SPLIT:, 0] == F(0.5)).all()  # the id stop keeps the tones apart
    for x in (SPLIT - 2, SPLIT - 1, SPLIT, SPLIT + 1):  # step 1: taps reach two columns, all within min(4, 2)
        assert (out[:, x, 0] > F(0.25)).all() and (out[:, x, 0] < F(0.5)).all(), x
    assert same(out[:, :SPLIT - 2], plain[:, :SPLIT - 2]).all() and same(out[:, SPLIT + 2:], plain[:, SPLIT + 2:]).all()
    # the second pass (step 2): r = 2 and 4; min(c) = 2 lets r = 2 cross, r = 4 not
    stats2 = dl.new_stats()
    dl.lens_pass(img, None, g, 1, WIDE, None, 4.0, 20.0, stats=stats2)
    rows = sum(min(H, H - 2 * dy) - max(0, -2 * dy) for dy in (-1, 0, 1))  # in-image rows of the taps with |dy| <= 1
    assert stats2["crossing"] == 2 * 2 * rows  # dx = +-1 (r = 2) from the two columns on each side of the edge


def test_the_minimum_keeps_a_sharp_side_untouched():
    g = step_guides()  # F = 10: the left side is in focus (c = 0), the right one is blurred (c = 4 * 30 / 40 = 3)
    c = dl.coc_radius(g, 4.0, 10.0)
    assert (c[:, :SPLIT] == 0).all() and (c[:, SPLIT:] == 3).all()
    img = two_tone(g)
    for variance in (None, 6.0):
        stats = dl.new_stats()
        p = dr.Params(iterations=3, sigma_color=100.0)
        out, _ = dl.denoise(img, g, p, variance, 4.0, 10.0, stats=stats)
        plain = dv.denoise(img, g, p, variance)[0] if variance else dr.denoise(img, g, p)
        assert stats["relaxed"] > 0 and stats["crossing"] == 0
        assert (dc.bits(out) == dc.bits(plain)).all()


def test_a_nan_t_relaxes_nothing():
    g = step_guides()
    g["t"][:, SPLIT:] = F(np.nan)  # the right side: c = NaN
    c = dl.coc_radius(g, 4.0, 20.0)
    assert np.isnan(c[:, SPLIT:]).all() and (c[:, :SPLIT] == 4).all()
    stats = dl.new_stats()
    dl.denoise(two_tone(g), g, WIDE, None, 4.0, 20.0, stats=stats)
    assert stats["crossing"] == 0 and stats["relaxed"] > 0  # (left to left taps are relaxed; none into or out of the NaN side)
    g["t"][:] = F(np.nan)
    stats = dl.new_stats()
    dl.denoise(two_tone(g), g, WIDE, None, 4.0, 20.0, stats=stats)
    assert stats["relaxed"] == 0


def test_a_miss_tap_uses_cock():
    g = step_guides(t_right=1e6, miss=True)  # the right side: c = 1.5 (1 - 20 / 1e6) ~ 1.49997; the misses: c = cocK = 1.5
    cocK = 1.5
    c = dl.coc_radius(g, cocK, 20.0)
    ids = g["id"]
    assert (c[ids == -1] == F(cocK)).all() and (c[ids == 256] < F(1.5)).all() and (c[ids == 256] > F(1.49)).all()
    stats = dl.new_stats()
    out, _ = dl.denoise(two_tone(g), g, WIDE, None, cocK, 20.0, stats=stats)
    # step 1, r <= 1.49997: the 8 neighbours.  Crossing taps: hit centre -> miss tap (column W - 5 -> W - 4) and the edge at SPLIT, where
    # the left side's c = 1.5 too (|10 - 20| / 10)
    expect = 0
    for y in range(H):
        for x in range(W):
            if ids[y, x] == -1:
                continue
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    qy, qx = y + dy, x + dx
                    if 0 <= qy < H and 0 <= qx < W and ids[qy, qx] != ids[y, x]:
                        expect += 1
    assert stats["crossing"] == expect > 0
    assert same(out[ids == -1], two_tone(g)[ids == -1]).all()  # a miss centre still passes through


def test_cock_of_the_host():
    k = dl.cock_of(1.0, 0.14, 20.0, 90, 0.41421357)
    want = 1.0 * (float(F(0.14)) / 2.0) / 20.0 * 90.0 / (2.0 * float(F(0.41421357)))
    assert k == F(want) and k.dtype == np.float32 and 0.37 < k < 0.39
    assert dl.cock_of(2.0, 0.14, 20.0, 90, -0.41421357) == F(2.0 * want)  # |invProj[5]|
    for args in [(0.0, 0.14, 20.0, 90, 0.4), (1.0, 0.0, 20.0, 90, 0.4), (1.0, -1.0, 20.0, 90, 0.4), (1.0, 0.14, 0.0, 90, 0.4),
                 (1.0, 0.14, 20.0, 90, 0.0), (3e38, 3e38, 1e-38, 32767, 1e-38)]:
        assert dl.cock_of(*args) == 0 and not np.signbit(dl.cock_of(*args)), args


# ------------------------------------------------------------------------------------------------ 3. passes that break one rule
def rule_max(r, cP, cQ, match, cocK, s, dx, dy):
    relaxed = bool(F(cocK) > 0) & ((r <= cP) | (r <= cQ))  # r <= max(c(p), c(q))
    return relaxed, relaxed | match


def rule_id_compared(r, cP, cQ, match, cocK, s, dx, dy):
    relaxed, _ = dl.relaxed_rule(r, cP, cQ, match, cocK, s, dx, dy)
    return relaxed, match  # the natural `if (id_q != id_p) continue;` left in front


def rule_tap_radius_only(r, cP, cQ, match, cocK, s, dx, dy):
    relaxed = bool(F(cocK) > 0) & (r <= cQ)
    return relaxed, relaxed | match


def rule_euclidean(r, cP, cQ, match, cocK, s, dx, dy):
    with np.errstate(all="ignore"):
        re = F(s) * np.sqrt(F(dx * dx + dy * dy))
    return dl.relaxed_rule(re, cP, cQ, match, cocK, s, dx, dy)


EDITS = {"max_instead_of_min": rule_max, "id_still_compared": rule_id_compared, "radius_of_the_tap_only": rule_tap_radius_only,
         "euclidean_distance": rule_euclidean}


@pytest.mark.parametrize("variance", [None, 6.0], ids=["fixed", "variance"])
@pytest.mark.parametrize("edit", sorted(EDITS))
def test_a_pass_that_breaks_one_rule_differs_on_the_recipes(edit, variance):
    """cocK = 2.5, F = 20: c = 2.5 on the left, 1.25 on the right — a diagonal tap across the edge has Chebyshev r = 1 <= 1.25 and
    Euclidean r = 1.41 > 1.25; a tap of r = 2 across it is within the larger radius only."""
    g = step_guides()
    total = 0
    for recipe in (di.NOISE, R("finite_specials", True), R("subnormal_block", True)):
        img = di.build(g["id"], recipe, 9)
        p = dr.Params(iterations=2)
        want, _ = dl.denoise(img, g, p, variance, 2.5, 20.0)
        again, _ = dl.denoise(img, g, p, variance, 2.5, 20.0, rule=dl.relaxed_rule)
        assert same(again, want).all()
        got, _ = dl.denoise(img, g, p, variance, 2.5, 20.0, rule=EDITS[edit])
        differ = int((~same(got, want).all(-1)).sum())
        print(f"{edit}, {'variance' if variance else 'fixed'}, {recipe.name}: differs from the restatement on {differ} of {H * W} pixels")
        assert differ > 0, recipe.name
        total += differ
    assert total > 0
