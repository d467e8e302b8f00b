"""The cases that tests/test_denoise_inputs_cpu.py (on synthetic guides) and tests/test_gpu_denoise_inputs.py (on the kernels' own
guides) both walk over the images of tests/denoise_inputs.py: shapes, the case tables of the two modes, the parameter extremes and
the temporal stage, as plain data; what a case expects (the restatements); the conditions, checked on the restatement's output alone,
that keep a case from hiding a failure; and the assertions that the arithmetic under the numpy restatements is IEEE (no flush to
zero) on the machine that runs them.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import denoise_reference as dr
import denoise_variance_reference as dv
from denoise_inputs import BLOCK, NOISE, F, Recipe, plan


# ------------------------------------------------------------------------------------------------ the arithmetic under the reference
TINY = F(1.17549435e-38)  # the smallest normal binary32


def assert_ieee_arithmetic():
    """numpy float32 on this machine keeps subnormals.  (1) float32(1e-39) * float32(0.5) == 5e-40.  (2) A restatement pass of either
    mode over subnormal_block on a 20x20 one-id plane returns subnormal, non-zero colours — means of the block's [1, 8] x 1e-39 — at the
    centres whose step-1 taps all lie in the block.  (With flush to zero in force the reference would be the side that departs from
    the definition.)"""
    assert F(1e-39) * F(0.5) == F(5e-40) and F(5e-40) != 0
    g = np.zeros((20, 20), dr.GUIDE_DTYPE)  # the head-on plane of tests/test_denoise_cpu.py: pos = (x, y, 0) / 10, t = 10
    yy, xx = np.meshgrid(np.arange(20, dtype=F), np.arange(20, dtype=F), indexing="ij")
    g["pos"][..., 0], g["pos"][..., 1], g["normal"][..., 2], g["t"] = xx * F(0.1), yy * F(0.1), F(1.0), F(10.0)
    pl = plan(g["id"], Recipe("subnormal_block"), 3)
    y0, y1, x0, x1, _ = pl.block
    assert (y1 - y0, x1 - x0) == (BLOCK, BLOCK)
    inner = (slice(y0 + 2, y1 - 2), slice(x0 + 2, x1 - 2))
    for out in (dr.atrous_pass(pl.image, g, 0, dr.Params()), dv.variance_pass(pl.image, dv.estimate(pl.image, g), g, 0, dr.Params(), 6.0)[0]):
        rgb = out[inner][..., :3]
        assert (rgb != 0).all() and (np.abs(rgb) < TINY).all()      # S / W is subnormal and not flushed
        assert (rgb >= F(1e-39)).all() and (rgb <= F(8e-39)).all()  # ... and a mean of the block's colours


# ------------------------------------------------------------------------------------------------ shapes and cases (plain data)
# (W, H).  Under the default camera the default scene shows at least two ids and hits on at least half of the pixels at each of them
# (checked on the CPU oracle by tests/test_denoise_inputs_cpu.py), so no shape needs a camera of its own.
SHAPES = (
    (131, 67),  # the existing anchor: many workgroups in both tilings, ragged right and top edge
    (65, 17),   # one past a 64-wide and a 16-high tile
    (64, 16),   # exact tiles
    (1, 40),    # every horizontal tap is off the image, the LDS halo's columns are all outside
    (40, 1),    # ... every vertical tap, the halo's rows
    (16, 5),
)


def scene_case(shape):
    """The first-hit case (tests/first_hit_cases.py) of a shape: the default scene under the default camera."""
    import first_hit_cases as fh
    assert shape in SHAPES
    return fh.Case(f"default_{shape[0]}x{shape[1]}", "default", shape[0], shape[1])


@dataclass(frozen=True)
class Case:
    shape: tuple                       # (W, H)
    recipe: Recipe
    variance: bool = False
    iterations: int = 5
    normal_log2_power: int = 5
    sigma_color: float = 0.5
    sigma_plane: float = 0.02
    sigma_variance: float = 6.0
    seed: int = 7

    @property
    def name(self):
        s = f"{'variance' if self.variance else 'fixed'}-{self.shape[0]}x{self.shape[1]}-{self.recipe.name}-it{self.iterations}"
        if self.normal_log2_power != 5:
            s += f"-pow{self.normal_log2_power}"
        for k, d in (("sigma_color", 0.5), ("sigma_plane", 0.02), ("sigma_variance", 6.0)):
            if getattr(self, k) != d:
                s += f"-{k}={getattr(self, k):g}"
        return s


def _cases():
    R = Recipe
    fs, sb = R("finite_specials", boundary=True), R("subnormal_block", boundary=True)
    shapes = list(SHAPES)
    out = []
    # fixed mode: finite_specials and subnormal_block with boundary_placement at iterations 1, 2, 3, 5, 6 and powers 0 and 7 on the anchor
    for rec in (fs, sb):
        for it in (1, 2, 3, 5, 6):
            for pw in (0, 7):
                out.append(Case((131, 67), rec, iterations=it, normal_log2_power=pw))
    # ... and on every other shape: each step's kernel (1 and 2: LDS, 4: direct) and full depth, one power each
    for k, sh in enumerate(shapes[1:]):
        for j, it in enumerate((1, 2, 3, 5)):
            out.append(Case(sh, fs if (j + k) % 2 == 0 else sb, iterations=it, normal_log2_power=(0, 7, 5)[(j + k) % 3]))
            out.append(Case(sh, sb if (j + k) % 2 == 0 else fs, iterations=it))
    # nonfinite_seed at iterations 1, 2, 3: pt_atrous_kernel<1 | 2 | 0, false> (iteration 3 is step 4 in the direct kernel)
    for it, val, ch in ((1, "nan", 1), (2, "+inf", 0), (3, "-inf", 2)):
        out.append(Case((131, 67), R("nonfinite_seed", value=val, channel=ch), iterations=it))
        # (65x17: three passes from the deepest pixel cover a quarter of the hits, so the third-pass seed sits in the smallest id)
        out.append(Case((65, 17), R("nonfinite_seed", value=val, channel=ch, where="deep" if it < 3 else "small"), iterations=it))
    out.append(Case((131, 67), R("nonfinite_seed", boundary=True, value="nan", channel=0), iterations=2))
    out.append(Case((65, 17), R("nonfinite_seed", boundary=True, value="+inf", channel=1), iterations=2))
    out.append(Case((1, 40), R("nonfinite_seed", value="nan"), iterations=1))  # (a line: 5 of its pixels after one pass, 13 after two)
    out.append(Case((40, 1), R("nonfinite_seed", value="-inf"), iterations=1))
    # one full-depth case whose seed sits in the smallest id of at least 9 pixels: the object bounds the spread
    out.append(Case((131, 67), R("nonfinite_seed", value="nan", where="small"), iterations=5))
    # variance mode: the same recipes at iterations 1, 2, 3, 5; flat, zero and nonfinite_seed at full depth
    for sh in ((131, 67), (65, 17)):
        for it in (1, 2, 3, 5):
            out.append(Case(sh, fs, True, iterations=it))
            out.append(Case(sh, sb, True, iterations=it))
    for k, sh in enumerate(shapes[2:]):
        for j, it in enumerate((1, 2, 3, 5)):
            out.append(Case(sh, fs if (j + k) % 2 == 0 else sb, True, iterations=it))
    for it, val, ch in ((1, "nan", 1), (2, "+inf", 0), (3, "-inf", 2), (5, "nan", 2)):
        out.append(Case((131, 67), R("nonfinite_seed", value=val, channel=ch), True, iterations=it))
    out.append(Case((131, 67), R("nonfinite_seed", boundary=True, value="-inf", channel=0), True, iterations=5))
    out.append(Case((65, 17), R("nonfinite_seed", value="+inf"), True, iterations=5))
    out.append(Case((131, 67), R("nonfinite_seed", value="+inf", where="small"), True, iterations=5))
    for sh in ((131, 67), (65, 17), (1, 40), (40, 1)):
        out.append(Case(sh, R("flat"), True, iterations=5))
        out.append(Case(sh, R("zero"), True, iterations=5))
    out.append(Case((131, 67), R("flat"), False, iterations=5))
    out.append(Case((65, 17), R("zero"), False, iterations=5))
    return out


CASES = _cases()

# Parameter extremes, all accepted by the setters, on the plain noise image at 65x17.  sigma_color 1e-40: inv_sigma = inf, every pixel
# passes through (0 * inf = NaN at the centre tap, NaN > 0 is false, so W is NaN or 0); 3e38: inv_sigma is subnormal.  sigma_variance
# 1e-25: k2 = 0; 1e-19: k2 subnormal; 1e19: k2 = 1e38; 3e38: k2 = inf.
EXTREMES = ([Case((65, 17), NOISE, sigma_color=v) for v in (1e-40, 1e-30, 3e38)]
            + [Case((65, 17), NOISE, sigma_plane=v) for v in (1e-40, 3e38)]
            + [Case((65, 17), NOISE, True, sigma_plane=v) for v in (1e-40, 3e38)]
            + [Case((65, 17), NOISE, True, sigma_variance=v) for v in (1e-25, 1e-19, 1e19, 3e38)])


@dataclass(frozen=True)
class TemporalCase:
    shape: tuple
    history: Recipe        # the image of epoch A (what the history holds)
    current: Recipe        # the image of epoch B
    n: int                 # frame index written with the image of epoch B
    max_history: int
    variance: bool = False
    n_history: int = 3     # frame index written with the image of epoch A
    iterations: int = 1    # fixed mode: one pass, so that what the blend makes non-finite (m' * Hc and n * C overflow from FLT_MAX) stays local
    seed: int = 11

    @property
    def name(self):
        return (f"temporal-{'variance' if self.variance else 'fixed'}-{self.shape[0]}x{self.shape[1]}-hist:{self.history.name}-cur:{self.current.name}"
                f"-n{self.n}-max{self.max_history}-it{self.iterations}")


def _temporal_cases():
    fs = Recipe("finite_specials", boundary=True, count=60)
    nf = Recipe("nonfinite_seed", value="nan", where="small")
    sb = Recipe("subnormal_block", boundary=True)
    out = []
    for hist, cur in ((fs, NOISE), (NOISE, fs), (fs, fs)):  # specials in the history only, in the current image only, in both
        for n in (0, 1, 1000):
            for mh in (1, 65535):
                out.append(TemporalCase((131, 67), hist, cur, n, mh))
    out.append(TemporalCase((131, 67), nf, NOISE, 1, 32))
    out.append(TemporalCase((131, 67), NOISE, nf, 1, 32))
    out.append(TemporalCase((65, 17), sb, sb, 1, 32))
    out.append(TemporalCase((65, 17), fs, nf, 2, 65535))
    out.append(TemporalCase((131, 67), fs, NOISE, 1, 32, iterations=0))  # the copy kernel on I
    out.append(TemporalCase((131, 67), fs, fs, 1, 32, variance=True, iterations=5))  # (the variance mode keeps a non-finite pixel to itself)
    return out


TEMPORAL_CASES = _temporal_cases()


# ------------------------------------------------------------------------------------------------ what a case expects, and whether it can fail
def params_of(case) -> dr.Params:
    return dr.Params(case.iterations, case.sigma_color, case.sigma_plane, case.normal_log2_power)


def restate(case, image, guides):
    """-> (expected image, expected V0 or None) of the case's mode and parameters."""
    if case.variance:
        return dv.denoise(image, guides, params_of(case), case.sigma_variance)
    return dr.denoise(image, guides, params_of(case)), None


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    """bit for bit, NaN == NaN"""
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


# "The filter changes more than half of the finite hit pixels" cannot be asked of the cases whose definition is the identity or nearly so.
# What is asked of them instead:
#   identity — flat, zero: the weighted mean of equal colours is that colour (0, and powers of two: w * c and every partial sum scale
#     exactly); sigma_color 1e-40: inv_sigma = inf, the centre tap's 0 * inf is NaN, W = 0.  No pixel changes.
#   narrow — sigma_color 1e-30 (inv_sigma >= 1e30: a^2 = inf for every du != 0) and sigma_variance 1e-25, 1e-19 (k2 * var <= 1e-38
#     vanishes beside 1e-8: a stop 1e-4 wide on the u scale, where the noise spans 0.27): nearly every pixel keeps its centre tap alone
#     and comes out as fl(fl(w C) / w), which misses C by an ulp only in the part of each binade of C where the product's ulp, divided
#     by w, exceeds half of C's (w = 9/64 at the centre of a plane).  Five passes over three channels: 0.19 and 0.23 of the
#     pixels on the synthetic plane.  Asked: more than a tenth — they must not silently become pure pass-through — and at most half.
# sigma_plane 1e-40 (a subnormal divisor: only taps with e = 0 count) is not among them: taps on a plane that faces the camera or
# lies along an axis have e = 0 exactly, and the filter changes 0.999 of the synthetic plane and 0.78 of the scene's 65x17 pixels.
def near_identity(case):
    """-> "identity", "narrow" or None"""
    if case.recipe.kind in ("flat", "zero") or case.sigma_color <= 1e-40:
        return "identity"
    if case.sigma_color <= 1e-30 or (case.variance and case.sigma_variance <= 1e-19):
        return "narrow"
    return None


def shares(image, want, ids):
    """-> (share of the hit pixels whose expected RGB is not finite, share of the finite ones that the restatement changes, hits)."""
    hit = ids >= 0
    finite = np.isfinite(want[..., :3]).all(-1)
    changed = ~same(want[..., :3], image[..., :3]).all(-1)
    nh, nf = int(hit.sum()), int((hit & finite).sum())
    return (float((hit & ~finite).sum()) / max(nh, 1), float((hit & finite & changed).sum()) / max(nf, 1), nh)


def assert_placement(name, recipe, ids, special):
    """A recipe's special pixels land on at least one hit pixel and, where boundary_placement puts them there, on one miss pixel."""
    if recipe.kind != "noise":
        assert (special & (ids >= 0)).any(), f"{name}: no special pixel on a hit pixel"
        if recipe.boundary and (ids == -1).any():
            assert (special & (ids == -1)).any(), f"{name}: no special pixel on a miss pixel"


def assert_case_can_fail(case, image, want, ids, special):
    """The conditions that keep a case from hiding a failure, on the restatement's output alone.  -> (non-finite share, changed share)"""
    nonfinite, changed, hits = shares(image, want, ids)
    assert hits > 0
    assert nonfinite <= 0.25, f"{case.name}: {nonfinite:.3f} of the hit pixels expect a non-finite colour: NaN == NaN compares nothing there"
    if case.iterations >= 1:
        kind = near_identity(case)
        if kind == "identity":
            assert changed == 0, f"{case.name}: the restatement changes {changed:.3f} of the pixels of an identity"
        elif kind == "narrow":
            assert 0.1 < changed <= 0.5, f"{case.name}: the restatement changes {changed:.3f} of the finite hit pixels"
        else:
            assert changed > 0.5, f"{case.name}: the restatement changes only {changed:.3f} of the finite hit pixels"
    assert_placement(case.name, case.recipe, ids, special)
    return nonfinite, changed


def assert_temporal_case_can_fail(tc, recipe, image, want_I, want_out, ids, special):
    """The same conditions for one epoch of a temporal case, whose image was built from `recipe`: at most a quarter of the hit pixels may
    expect a non-finite integrated colour, or a non-finite output; with iterations >= 1 the stage and the filter together change more
    than half of the finite hit pixels; the placement.  -> (non-finite share of I, of the output, changed share)"""
    nonfinite_I = shares(image, want_I, ids)[0]
    nonfinite, changed, hits = shares(image, want_out, ids)
    assert hits > 0
    assert max(nonfinite_I, nonfinite) <= 0.25, f"{tc.name}: {nonfinite_I:.3f} of the hit pixels expect a non-finite I, {nonfinite:.3f} a non-finite output"
    if tc.iterations >= 1:
        assert changed > 0.5, f"{tc.name}: the stage and the filter change only {changed:.3f} of the finite hit pixels"
    assert_placement(tc.name, recipe, ids, special)
    return nonfinite_I, nonfinite, changed
