"""The "pt-f32" contract where it is made: the device code object of csrc/pt_math.hpp's primitives and csrc/pt_device.hpp's leaf functions
(tools/pt_device_probe.hip, built with the library's own flags by native.build_probe) against the CPU oracle, word for word, on the grids
of tests/math_probe_cases.py — and four exhaustive sweeps whose reference is computed on the device.

  grid D (what the integrator can produce): the oracle returns no NaN, words must be equal, no row may differ.
  grid W (every exponent, denormals, zeros, infinities, NaNs of both kinds, 2^20 random words) and the edge rows of the vector functions:
         the project's rule (degenerate_cases.same_colour) — words equal, or both NaN; the NaN-only matches are counted and printed.
  What the C language leaves open is taken out by an explicit predicate on the INPUT, never by a wider rule: pt_sincos beyond |a| < 2^30
  (the quadrant is (int)k), f_min / f_max of zeros of opposite sign and of signalling NaNs (math_probe_cases.minmax_comparable).

The control (test_flushed_denormals_are_seen) runs the same comparisons on the same source built with -fgpu-flush-denormals-to-zero, and
requires them to FAIL: keeping denormals is part of the contract, and a grid that cannot see it broken does not test it.

tests/test_math_probe_cpu.py runs the same rows on a host build of the same source, so grids and references are known to be sound."""
import numpy as np
import pytest

import math_probe_cases as mc

pytestmark = pytest.mark.gpu


def _load(pkg, name):
    pkg.native._share_torch_hip_runtime()  # (the HIP runtime the rest of the suite uses, whichever test comes first)
    return mc.Probe(pkg.native.build_probe(name))


@pytest.fixture(scope="module")
def probe(pkg):
    return _load(pkg, "probe")


@pytest.fixture(scope="module")
def probe_ftz(pkg):
    return _load(pkg, "probe_ftz")


_GRIDS = {"D": mc.grid_d, "W": mc.grid_w_for, "edge": mc.grid_edge}
_REFS = {}


def want_of(oracle, name, kind):
    """the reference of one grid, computed once and shared (read-only)"""
    if (name, kind) not in _REFS:
        ref = mc.reference(oracle, name, _GRIDS[kind](name))
        ref.setflags(write=False)
        _REFS[name, kind] = ref
    return _REFS[name, kind]


def _float_columns(name, out):
    return {"to_unorm8": out[:, :0], "pcg_hash": out[:, :0], "pixel_seed": out[:, :0], "rand01": out[:, :1], "cosine_sample_hemisphere": out[:, :3]}.get(name, out)


def differing(probe, oracle, name, kind):
    """(rows of the grid, rows that differ, rows that match only as NaNs, description of the first differing row)"""
    rows, want = _GRIDS[kind](name), want_of(oracle, name, kind)
    got = probe.eval(name, rows)
    if kind == "D":
        assert not np.isnan(mc.floats(_float_columns(name, want))).any(), f"{name}: the oracle returns a NaN on its domain grid"
        ne = (got != want).any(-1)
        bad, nan_only, first = int(ne.sum()), 0, (int(np.flatnonzero(ne)[0]) if ne.any() else -1)
    else:
        bad, nan_only, first = mc.compare(got, want)
    return len(rows), bad, nan_only, mc.describe(name, rows, got, want, first)


def hold(probe, oracle, names, kinds=("D", "W")):
    failures = []
    for name in names:
        for kind in kinds:
            if (kind == "D" and name not in mc.ON_GRID_D) or (kind == "W" and name not in mc.ON_GRID_W) or (kind == "edge" and name not in mc.VECTOR_GRIDS):
                continue
            n, bad, nan_only, what = differing(probe, oracle, name, kind)
            print(f"{name:26s} grid {kind:4s} {n:9d} rows, {bad} differ, {nan_only} match only as NaNs")
            if bad:
                failures.append(f"grid {kind}: {bad} of {n} rows differ; {what}")
    assert not failures, "\n".join(failures)


def test_reciprocal_roots_and_division(probe, oracle):
    """f_rcp, f_rsqrt, pt_sqrt (the Newton sequences) against the oracle's; f_sqrt and f_div_ieee (the compiler's expansions of sqrt and /)
    against numpy float32, correctly rounded: denormal operands and results included"""
    hold(probe, oracle, ["f_rcp", "f_rsqrt", "pt_sqrt", "f_sqrt", "f_div_ieee"])


def test_min_max_mix(probe, oracle):
    hold(probe, oracle, ["f_min", "f_max", "f_mix"])


def test_sincos(probe, oracle):
    """every angle hemisphere_draws can form, a = (k 2^-24) * 2 * PI for k = 0 .. 2^24 (rand01 == 1.0), and grid W where |a| < 2^30"""
    hold(probe, oracle, ["pt_sincos"])


def test_exp_log_pow5(probe, oracle):
    """both forms of pt_exp (the branched one and the selected one the default kernel runs) on [-104, 88.73] with the floats around every
    threshold and the first denormal result; pt_log on [0.0031308, 1]; pt_pow5; all of them on grid W"""
    hold(probe, oracle, ["pt_exp", "pt_exp_selected", "pt_log", "pt_pow5"])


def test_tone_map_chain(probe, oracle):
    """aces_film, linear_to_inverse_gamma(v, 2.4), to_unorm8 (the floats around every rounding boundary (b + 0.5) / 255)"""
    hold(probe, oracle, ["aces_film", "linear_to_inverse_gamma", "to_unorm8"])


def test_rng(probe, oracle):
    """pcg_hash (word and seed), rand01 on the seeds that hash to the words around every round-to-even tie of the 24-bit conversion and to
    0xFFFFFFFF (rand01 == 1.0), pixel_seed at the corners of the largest image and the largest frame index"""
    hold(probe, oracle, ["pcg_hash", "rand01", "pixel_seed"])


def test_vector_leaf_functions(probe, oracle):
    """v_normalize, f_reflect, f_refract (both sides of total internal reflection), fresnel_schlick: unit vectors with zero and denormal
    components, normal and grazing incidence; the degenerate rows (zero vectors, non-finite components) under the NaN rule"""
    hold(probe, oracle, ["v_normalize", "f_reflect", "f_refract", "fresnel_schlick"], ("D", "edge"))


def test_hemisphere_sampling(probe, oracle):
    """hemisphere_direction with z = +-1 (r = 0) and a sample that cancels the normal; cosine_sample_hemisphere from seeds whose first or
    second draw is exactly 1.0 (direction and seed out)"""
    hold(probe, oracle, ["hemisphere_direction", "cosine_sample_hemisphere"], ("D", "edge"))


def test_cuboid_normal(probe, oracle):
    """cuboid_normal selects its scale where the oracle computes f_rsqrt(dot(n, n)): on and off the faces of three boxes, within two floats
    of the EPSILON step, NaN and infinite points; and (sweep 4) on all 64 combinations of components -1, -0, +0, +1 against
    v_scale(n, f_rsqrt(v_dot(n, n))) computed on the device"""
    hold(probe, oracle, ["cuboid_normal"], ("D", "edge"))
    r = probe.sweep("cuboid_scale", 0, 64)
    assert r["mismatches"] == 0, f"combinations {r['offenders']} differ from the computed scale"


def test_sweep_selected_exp_is_the_branched_exp(probe):
    """sweep 1: pt_exp<true>(x) against pt_exp<false>(x) for all 2^32 words — "the same value for every input" (csrc/pt_math.hpp)"""
    r = probe.sweep("exp_selected", 0, 2 ** 32)
    print(f"pt_exp<true> against pt_exp<false>, 2^32 words: {r['mismatches']} mismatches")
    assert r["mismatches"] == 0, "first offending words: " + " ".join(f"{w:#010x}" for w in r["offenders"])


def test_sweep_rand01_conversion_rounds_to_nearest_even(probe):
    """sweep 2: rand01 of all 2^32 seeds (pcg_hash is a bijection: all 2^32 words) against a round-to-nearest-even uint32 -> binary32
    conversion written in integer arithmetic, times 2^-32"""
    r = probe.sweep("rand01", 0, 2 ** 32)
    print(f"rand01 against the integer conversion, 2^32 seeds: {r['mismatches']} mismatches")
    assert r["mismatches"] == 0, "first offending seeds: " + " ".join(f"{w:#010x}" for w in r["offenders"])


def test_sweep_accuracy_of_reciprocal_and_roots(probe, oracle):
    """sweep 3: every float with |x| in [1e-30, 1e30] — the range test_contract_reciprocal_root_accuracy samples — against a
    double-precision value computed on the device, in float ulps, inside the project's bounds 0.52 (f_rcp, both signs), 1.75 (f_rsqrt),
    0.502 (pt_sqrt).  First the double-precision divide and square root themselves: equal to numpy float64 on grid W."""
    w = mc.grid_w().reshape(-1, 1)
    for name in ("ref_rcp", "ref_rsqrt", "ref_sqrt"):
        got = np.ascontiguousarray(probe.eval(name, w)).view(np.uint64)
        want = np.ascontiguousarray(mc.reference(oracle, name, w)).view(np.uint64)
        ok = (got == want) | (np.isnan(got.view(np.float64)) & np.isnan(want.view(np.float64)))
        assert ok.all(), f"{name}: {int((~ok).sum())} rows differ from numpy float64, first at word {int(w[np.flatnonzero(~ok.ravel())[0], 0]):#010x}"
    lo, hi = mc.bits(1e-30), mc.bits(1e30)
    failures = []
    for name, first in (("f_rcp", lo), ("f_rcp", lo | 0x80000000), ("f_rsqrt", lo), ("pt_sqrt", lo)):
        r = probe.sweep(name, first, hi - lo + 1)
        print(f"{name}{' (negative)' if first >> 31 else ''}: {hi - lo + 1} words, largest error {r['max_error']:.6f} ulp at {r['max_error_word']:#010x}, "
              f"{r['mismatches']} above {mc.ULP_BOUNDS[name]}: " + " ".join(f"{x:#010x}" for x in r["offenders"]))
        if r["mismatches"] or not r["max_error"] <= mc.ULP_BOUNDS[name]:
            failures.append(f"{name}: {r}")
    assert not failures, "\n".join(failures)


def test_flushed_denormals_are_seen(probe_ftz, oracle):
    """the control: the same source built with -fgpu-flush-denormals-to-zero must DIFFER from the oracle on pt_exp's domain grid (both
    forms) and on f_div_ieee's rows of grid W; pt_sqrt's rows are reported"""
    differed = []
    for name, kind in (("pt_exp", "D"), ("pt_exp_selected", "D"), ("f_div_ieee", "W"), ("pt_sqrt", "W")):
        n, bad, nan_only, what = differing(probe_ftz, oracle, name, kind)
        print(f"flushed build: {name:16s} grid {kind} {bad} of {n} rows differ; {what}")
        if bad:
            differed.append(name)
    print("flushed build differs on:", ", ".join(differed))
    assert {"pt_exp", "pt_exp_selected", "f_div_ieee"} <= set(differed), differed
