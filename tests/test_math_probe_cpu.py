"""The math probe without a GPU: tools/pt_device_probe.hip compiled for the HOST (hipcc --cuda-host-only -DPT_PROBE_HOST, the library's
arithmetic flags, as tests/test_bounce_regions_cpu.py compiles its probe) and compared with the oracle on every grid of
tests/math_probe_cases.py, under the rule the GPU test uses.  It shows that the grids and the references are sound before a GPU is
involved, and pins what was measured when the grids were made: the sequences of csrc/pt_math.hpp and the leaf functions of
csrc/pt_device.hpp, compiled by clang for x86, give the oracle's words (gcc) on every row, NaN payloads aside.

Both headers compile for the host (what csrc/pt_device.hpp holds of wave intrinsics and inline assembly sits in inline functions the
probe does not call), so no function is left to the GPU test alone."""
import subprocess

import numpy as np
import pytest

import math_probe_cases as mc


@pytest.fixture(scope="module")
def probe(pkg, tmp_path_factory):
    lib = tmp_path_factory.mktemp("mathprobe") / "libprobe_host.so"
    flags = [f for f in pkg.native.HIPCC_FLAGS if not f.startswith("--offload-arch")]
    p = subprocess.run([pkg.native.hipcc_path(), "-x", "hip", "--cuda-host-only", "-DPT_PROBE_HOST", *flags, "-I", pkg.native.CSRC,
                        pkg.native.PROBE_SRC, "-o", str(lib)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    return mc.Probe(str(lib))


def _float_columns(name, out):
    return {"to_unorm8": out[:, :0], "pcg_hash": out[:, :0], "pixel_seed": out[:, :0], "rand01": out[:, :1], "cosine_sample_hemisphere": out[:, :3]}.get(name, out)


@pytest.mark.parametrize("name", mc.ON_GRID_D)
def test_domain_grid_equals_the_oracle(probe, oracle, name):
    """grid D: the oracle returns no NaN, and the host build of the headers returns the oracle's words on every row"""
    rows = mc.grid_d(name)
    want = mc.reference(oracle, name, rows)
    assert not np.isnan(mc.floats(_float_columns(name, want))).any(), f"{name}: the oracle returns a NaN on its domain grid"
    got = probe.eval(name, rows)
    bad = int((got != want).any(-1).sum())
    assert bad == 0, f"{bad} of {len(rows)} rows differ; " + mc.describe(name, rows, got, want, int(np.flatnonzero((got != want).any(-1))[0]))


@pytest.mark.parametrize("name", mc.ON_GRID_W)
def test_word_grid_equals_the_oracle(probe, oracle, name):
    """grid W: words equal or both NaN (NaN-only matches counted: clang and gcc keep different payloads)"""
    rows = mc.grid_w_for(name)
    want = mc.reference(oracle, name, rows)
    got = probe.eval(name, rows)
    bad, nan_only, first = mc.compare(got, want)
    print(f"{name}: {len(rows)} rows, {nan_only} match only as NaNs")
    assert bad == 0, f"{bad} of {len(rows)} rows differ; " + mc.describe(name, rows, got, want, first)


@pytest.mark.parametrize("name", list(mc.VECTOR_GRIDS))
def test_edge_rows_equal_the_oracle(probe, oracle, name):
    rows = mc.grid_edge(name)
    want = mc.reference(oracle, name, rows)
    got = probe.eval(name, rows)
    bad, nan_only, first = mc.compare(got, want)
    assert bad == 0, mc.describe(name, rows, got, want, first)
    assert np.isnan(mc.floats(_float_columns(name, want))).any()  # (the rows are there because their result is a NaN)


@pytest.mark.parametrize("name", ["f_refract", "cuboid_normal", "cosine_sample_hemisphere"])
def test_vector_grids_reach_their_decisions(oracle, name):
    """the grids built to put a decision on both sides do so (on the oracle)"""
    want = mc.reference(oracle, name, mc.grid_d(name))
    if name == "f_refract":  # both sides of total internal reflection, on the rows built to straddle k == 0
        tail = mc.floats(want[-8 * 129:]).reshape(8, 129, 3)
        tir = (tail == 0).all(-1)
        assert (tir.any(1) & ~tir.all(1)).all(), "a critical-angle block lies entirely on one side of k == 0"
    if name == "cuboid_normal":  # every count of faces hit: none (n = 0 is an edge row), one, two, three
        q = np.round((mc.floats(want).astype(np.float64) ** 2).sum(-1), 3)
        assert set(np.unique(np.count_nonzero(mc.floats(want), axis=1))) >= {1, 2, 3} and np.allclose(q, 1.0, atol=1e-3)
    if name == "cosine_sample_hemisphere":  # the seeds built to draw rand01 == 1.0 do
        one = mc.unhash(np.array([0xFFFFFFFF], np.uint64))
        assert float(oracle.rand01_array(one)[0][0]) == 1.0 and float(oracle.rand01_array(mc.seed_before(one))[0][0]) != 1.0
        assert oracle.pcg_hash_array(mc.seed_before(one))[1][0] == one[0]


def test_hemisphere_direction_reference_is_the_oracles(oracle):
    """the oracle has hemisphere_direction only inside cosine_sample_hemisphere: the reference put together from its pt_sqrt, sincos and
    normalize (math_probe_cases.hemisphere_direction_reference), fed the two draws, gives cosine_sample_hemisphere's words and seeds on
    that function's whole grid, the seeds that draw exactly 1.0 and the edge rows included"""
    for rows in (mc.grid_d("cosine_sample_hemisphere"), mc.grid_edge("cosine_sample_hemisphere")):
        n, seeds = mc.floats(rows[:, :3].copy()), rows[:, 3].copy()
        z, a, after = mc.hemisphere_draws_reference(oracle, seeds)
        want, want_seed = oracle.cosine_sample_hemisphere_array(n, seeds)
        bad, _, first = mc.compare(mc.words(mc.hemisphere_direction_reference(oracle, n, z, a)), mc.words(want))
        assert bad == 0 and np.array_equal(after, want_seed), (bad, first)


def test_rand01_grid_reaches_the_ties(oracle):
    """unhash() inverts pcg_hash: the seeds of the rand01 grid hash to the tie words they were made from, 0xFFFFFFFF among them"""
    ties = mc.rand01_tie_words()
    word, _ = oracle.pcg_hash_array(mc.unhash(ties))
    assert np.array_equal(word, ties) and 0xFFFFFFFF in ties
    v, _ = oracle.rand01_array(mc.unhash(np.array([0xFFFFFFFF, 0xFFFFFF80, 0xFFFFFF7F], np.uint64)))
    assert v[0] == 1.0 and v[1] == 1.0 and v[2] == np.float32(1.0 - 2.0 ** -24)  # (the tie rounds to even: up to 1.0)


def test_sweeps_on_the_host(probe):
    """the sweep code of the probe (pt_exp<true> against pt_exp<false>; rand01 against the integer conversion; the ulp measure; the 64
    combinations of cuboid_normal's selected scale), on
    slices small enough for a CPU: around both zeros, the thresholds of pt_exp, the top of the word range, and one binade for the
    accuracy sweeps.  The exhaustive runs are the GPU's."""
    for first, count in ((0, 2 ** 18), (0x80000000 - 2 ** 17, 2 ** 18), (mc.bits(88.72283935546875) - 2 ** 17, 2 ** 18),
                         (mc.bits(-104.0) - 2 ** 17, 2 ** 18), (0x7F800000 - 2 ** 17, 2 ** 18), (2 ** 32 - 2 ** 18, 2 ** 18)):
        r = probe.sweep("exp_selected", first, count)
        assert r["mismatches"] == 0, (hex(first), [hex(w) for w in r["offenders"]])
    for first in (0, 2 ** 24 - 2 ** 17, 2 ** 31 - 2 ** 17, 2 ** 32 - 2 ** 18):
        r = probe.sweep("rand01", first, 2 ** 18)
        assert r["mismatches"] == 0, (hex(first), [hex(w) for w in r["offenders"]])
    for name in ("f_rcp", "f_rsqrt", "pt_sqrt"):
        r = probe.sweep(name, mc.bits(1.0), 2 ** 22)  # [1, 1.5)
        print(f"{name}: largest error on [1, 1.5) {r['max_error']:.4f} ulp at word {r['max_error_word']:#010x}")
        assert r["mismatches"] == 0 and 0.3 < r["max_error"] <= mc.ULP_BOUNDS[name], r
    assert probe.sweep("cuboid_scale", 0, 64)["mismatches"] == 0


def test_sweep_reference_conversion_is_round_to_nearest_even(probe, oracle):
    """the integer conversion the rand01 sweep compares with is itself right: numpy's uint32 -> float32 (round to nearest even) times 2^-32
    on the tie words — through the rand01 rows, which the sweep code accepted above"""
    seeds = mc.unhash(mc.rand01_tie_words())
    got = mc.floats(probe.eval("rand01", seeds.reshape(-1, 1))[:, 0])
    want = mc.rand01_tie_words().astype(np.float32) * np.float32(2.0 ** -32)
    assert np.array_equal(mc.words(got), mc.words(want))
    r = probe.sweep("rand01", int(seeds[0]), 1)
    assert r["mismatches"] == 0
