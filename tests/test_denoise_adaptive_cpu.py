"""The adaptive sampler's noise as the denoiser's noise source without a GPU (pt_denoise_set_adaptive_noise,
pt_denoise_read_variance_used): the ABI (header, exports of the product and the diagnostic builds, argument checks without a handle,
Python and C++ harness) and the properties of the numpy restatement (tests/denoise_adaptive_reference.py) that
tests/test_gpu_denoise_adaptive.py compares the kernel with, bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import adaptive_reference as ar
import denoise_adaptive_reference as da
import denoise_reference as dr
import denoise_variance_reference as dv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355pt.h")
SYMBOLS = ["pt_denoise_set_adaptive_noise", "pt_denoise_read_variance_used"]
METHODS = ["SetDenoiseAdaptiveNoise", "DenoiseVarianceUsed"]
H, W = 24, 40  # 3 x 5 adaptive tiles
F = np.float32


# ------------------------------------------------------------------------------------------------ ABI
def test_header_declares_the_two_calls_beside_the_moments_and_cites_the_host_code_they_serve():
    text = open(HEADER).read()
    h = r"PT_API\s+int\s+{}\s*\(\s*pt_handle\s+h\s*,\s*{}\s*\)\s*;"
    assert re.search(h.format("pt_denoise_set_adaptive_noise", r"int\s+enable\s*,\s*int\s+prior_samples"), text)
    assert re.search(h.format("pt_denoise_read_variance_used", r"float\s*\*\s*dst\s*,\s*size_t\s+row_pitch_bytes"), text)
    for name in SYMBOLS:
        comment = text[:text.index(f"PT_API int {name}(")].rsplit("/*", 1)[1]
        assert "MainWindow.cs:49-63" in comment and "ScreenEffect.cs:29-37" in comment, name
    assert text.index("PT_API int pt_denoise_noise_level(") < text.index("PT_API int pt_denoise_set_adaptive_noise(") < text.index("PT_API int pt_adaptive_set_params(")
    comment = text[:text.index("PT_API int pt_denoise_set_adaptive_noise(")].rsplit("/*", 1)[1]
    assert re.search(r"Defaults\s+0,\s+8\b", comment)


def test_header_compiles_as_c99_and_a_c_caller_links_the_names(tmp_path):
    src = tmp_path / "adaptive_noise.c"
    src.write_text('#include "mi355pt.h"\n'
                   "int show(pt_handle h, float *var0)\n{\n"
                   "    if (pt_denoise_set_mode(h, PT_DENOISE_VARIANCE, 6.0f) != PT_OK || pt_denoise_set_adaptive_noise(h, 1, 8) != PT_OK) return -1;\n"
                   "    if (pt_adaptive_render(h, 4) != PT_OK || pt_denoise_render(h, 0) != PT_OK) return -2;\n"
                   "    return pt_denoise_read_variance_used(h, var0, 0) == PT_OK;\n}\n")
    p = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "adaptive_noise.o")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_product_and_diagnostic_builds_export_the_two_symbols(pkg, native_lib):
    assert set(SYMBOLS) <= set(pkg.native.declared_symbols())
    assert "pt_denoise_adaptive.hip" in pkg.native.SOURCES
    paths = [pkg.native.LIB_PATH]
    for variant in pkg.native.VARIANTS:
        pkg.native.build_variant(variant)  # (rebuilt when older than the sources)
        paths.append(pkg.native.variant_path(variant))
    for path in paths:
        lib = C.CDLL(path)
        missing = [s for s in SYMBOLS if not hasattr(lib, s)]
        assert not missing, f"{path} lacks {missing}"


def test_calls_fail_loudly_without_a_handle(pkg, native_lib):
    N = pkg.native
    assert native_lib.pt_denoise_set_adaptive_noise.argtypes == [C.c_void_p, C.c_int, C.c_int]
    assert native_lib.pt_denoise_read_variance_used.argtypes == [C.c_void_p, C.POINTER(C.c_float), C.c_size_t]
    buf = (C.c_float * 16)()
    assert native_lib.pt_denoise_set_adaptive_noise(None, 1, 8) == N.PT_E_BAD_HANDLE
    assert native_lib.pt_denoise_read_variance_used(None, buf, 0) == N.PT_E_BAD_HANDLE


def test_python_and_cpp_harness(pkg):
    host = open(os.path.join(pkg.native.HERE, "host", "pt_host.hpp")).read()
    for method in METHODS:
        assert callable(getattr(pkg.PathTracer, method, None)), method
        assert re.search(rf"\b{method}\s*\(", host), method
    demo = open(os.path.join(pkg.native.HERE, "host", "pt_host_demo.cpp")).read()
    assert re.search(r"\bSetDenoiseAdaptiveNoise\s*\(", demo)
    assert os.path.exists(pkg.native.build_host_demo())  # (compiles the two methods)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in SYMBOLS:
        assert re.search(r"\[DllImport\(Lib\)\][^\n]*\b" + name + r"\s*\(", integration), name


# ------------------------------------------------------------------------------------------------ the restatement's own properties
def records(k, k0):
    """(H / 8, W / 8) tile records from per-tile k (an array or a number) and k0"""
    r = np.zeros((H // 8, W // 8), ar.TILE_DTYPE)
    r["k"], r["k0"], r["n"] = k, k0, 64
    return r


def some_v0(seed=0):
    return np.random.default_rng(seed).uniform(1e-4, 1e-2, (H, W)).astype(F)


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def test_uniform_counts_and_a_constant_estimate_give_the_closed_form():
    """k = 16, k0 = 8 everywhere (j = 8), c = 2^-6, e = c / k = 2^-10: e kf = c exactly, the window sum is cnt c with cnt = 4, 6 or 9,
    exact in binary32, S = c, Et = c / 16 = 2^-10, and var_0 = ((8 2^-10) + (8 V0)) / 16 for whatever V0 holds."""
    c, k, j = F(2.0 ** -6), 16, 8
    e = np.full((H, W), c / F(k), F)
    ids = np.zeros((H, W), np.int32)
    v0 = some_v0()
    for prior in (8, 32):
        got = da.blend(e, records(k, k - j), v0, ids, prior)
        want = ((F(j) * (c / F(k))) + (F(prior) * v0)) / (F(j) + F(prior))
        assert got.dtype == np.float32 and _same(got, want.astype(F)), prior
    assert da.DEFAULT_PRIOR_SAMPLES == 8


def test_a_neighbour_across_a_tile_border_tells_its_per_sample_variance():
    """Tile columns 0-1 hold k = 4, columns 2-4 hold k = 16, the per-sample variance is s = 2^-4 everywhere (e = s / k, exact): the
    rescaled window gives Et = s / k_p on both sides of the border at x = 16, the plain window mean of e does not."""
    s = F(2.0 ** -4)
    k = np.where(np.arange(W // 8) < 2, 4, 16)[None, :].repeat(H // 8, 0)
    rec = records(k, 1)
    kp, jp = da.pixel_counts(rec, (H, W))
    assert set(np.unique(kp[:, :16])) == {4} and set(np.unique(kp[:, 16:])) == {16}
    e = (s / kp.astype(F)).astype(F)
    ids = np.zeros((H, W), np.int32)
    S = da.window_mean(da.per_sample(e, rec), ids)
    assert _same(S, np.full((H, W), s, F))
    et = S / kp.astype(F)
    assert _same(et, e)  # s / k_p everywhere, the two border columns included
    plain = da.window_mean(e, ids)
    assert (plain[:, 15] != e[:, 15]).all() and (plain[:, 16] != e[:, 16]).all()  # (what a window that ignores the counts would read)
    assert _same(plain[:, :15], e[:, :15]) and _same(plain[:, 17:], e[:, 17:])
    zero = np.zeros((H, W), F)
    got = da.blend(e, rec, zero, ids, 8)
    want = ((jp.astype(F) * e) + (F(8.0) * zero)) / (jp.astype(F) + F(8.0))
    assert _same(got, want.astype(F))


def test_a_miss_and_a_tile_without_statistics_keep_v0():
    """id = -1, and k - k0 <= 0 (0 and negative: a record a host could not make, which the rule covers all the same)"""
    k0 = np.full((H // 8, W // 8), 4)
    k0[0, 0], k0[1, 2] = 8, 9
    rec = records(8, k0)
    ids = np.zeros((H, W), np.int32)
    ids[:, 30:] = -1
    ids[20:, :] = 7
    e = np.random.default_rng(1).uniform(1e-4, 1e-2, (H, W)).astype(F)
    e[:8, :8] = 0  # (the sampler's e while k - k0 <= 0)
    e[8:16, 16:24] = 0
    v0 = some_v0(2)
    got = da.blend(e, rec, v0, ids, 8)
    keep = (ids == -1)
    keep[:8, :8] = True
    keep[8:16, 16:24] = True
    assert _same(got[keep], v0[keep])
    assert (got[~keep] != v0[~keep]).all()
    # a neighbour of such a tile still reads the tile's cells (e = 0 there): no rule of their own
    S = da.window_mean(da.per_sample(e, rec), ids)
    y, x = 3, 8
    want = F(0.0)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            want = want + e[y + dy, x + dx] * F(8.0)
    assert S[y, x] == want / F(9.0) and e[y, x - 1] == 0


def test_an_infinite_estimate_reaches_exactly_the_3x3_window_of_its_id():
    rec = records(16, 8)
    ids = np.zeros((H, W), np.int32)
    ids[:, 21:] = 3  # an id edge right of the pixel
    e = np.random.default_rng(3).uniform(1e-4, 1e-2, (H, W)).astype(F)
    e[10, 20] = np.inf
    v0 = some_v0(4)
    got = da.blend(e, rec, v0, ids, 8)
    want = np.zeros((H, W), bool)
    want[9:12, 19:21] = True  # (column 21 is another id)
    assert (np.isposinf(got) == want).all() and np.isfinite(got[~want]).all() and not np.isnan(got).any()


def test_a_nan_in_v0_stays_nan_and_nothing_else_becomes_one():
    rec = records(16, 8)
    ids = np.zeros((H, W), np.int32)
    ids[:4] = -1
    e = np.random.default_rng(5).uniform(1e-4, 1e-2, (H, W)).astype(F)
    v0 = some_v0(6)
    v0[2, 5] = v0[12, 17] = np.nan
    got = da.blend(e, rec, v0, ids, 8)
    assert (np.isnan(got) == np.isnan(v0)).all()
    # and the filter's own arithmetic, not a select, carries it: +inf e with a NaN V0 is NaN as well
    e[12, 17] = np.inf
    got = da.blend(e, rec, v0, ids, 8)
    assert np.isnan(got[12, 17]) and np.isposinf(got[11, 16])


def test_float32_stays_within_fourteen_roundings_of_float64():
    """Every term is positive, so nothing cancels: var_0 goes through at most 14 roundings in sequence — the product e kf, up to 8
    additions of the window sum, / cnt, / kf, jf Et, K0 V0 (beside it, not behind it), their sum and the final quotient; jf + K0 and the
    conversions are exact — each a relative 2^-24 at most: (1 + 2^-24)^14 - 1 < 15 2^-24.  Inputs well inside the normal range."""
    rng = np.random.default_rng(7)
    k = rng.integers(5, 97, (H // 8, W // 8))
    rec = records(k, 1)
    ids = rng.integers(0, 3, (H, W)).astype(np.int32)
    e = rng.uniform(1e-5, 1e-2, (H, W)).astype(F)
    v0 = some_v0(8)
    got = da.blend(e, rec, v0, ids, 8).astype(np.float64)
    kp, jp = da.pixel_counts(rec, (H, W))
    x = e.astype(np.float64) * kp
    s, cnt = np.zeros((H, W)), np.zeros((H, W))
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            sh = dv._shift(H, W, dy, dx)
            P, Q = sh
            visit = ids[Q] == ids[P]
            s[P] += np.where(visit, x[Q], 0.0)
            cnt[P] += visit
    want = (jp * (s / cnt / kp) + 8.0 * v0.astype(np.float64)) / (jp + 8.0)
    rel = np.abs(got - want) / want
    print(f"float32 against float64: max relative error {rel.max() / 2.0 ** -24:.2f} x 2^-24 (bound 15)")
    assert rel.max() < 15 * 2.0 ** -24


def test_the_filter_runs_the_existing_passes_on_var_0():
    """iterations = 0: a copy; with e = 0 everywhere and prior_samples large against j, var_0 -> V0 (K0 V0) / (j + K0) and the result is
    the passes of the variance mode on it; var0 handed in is used as it is."""
    g = np.zeros((H, W), dr.GUIDE_DTYPE)
    yy, xx = np.meshgrid(np.arange(H, dtype=F), np.arange(W, dtype=F), indexing="ij")
    g["pos"][..., 0], g["pos"][..., 1] = xx * F(0.1), yy * F(0.1)
    g["normal"][:] = np.asarray((0.0, 0.0, 1.0), F)
    g["t"] = F(10.0)
    c = np.ones((H, W, 4), F)
    c[..., :3] = np.random.default_rng(9).uniform(0.2, 0.8, (H, W, 1)).astype(F)
    rec = records(8, 8)  # k - k0 = 0: var_0 = V0, so the filter is the variance mode itself
    e = np.zeros((H, W), F)
    out, v0, var0 = da.denoise(c, g, e, rec)
    want, want_v0 = dv.denoise(c, g)
    assert _same(v0, want_v0) and _same(var0, v0) and _same(out, want)
    out0, none_v0, none_var0 = da.denoise(c, g, e, rec, dr.Params(iterations=0))
    assert _same(out0, c) and none_v0 is None and none_var0 is None
    rec = records(16, 8)
    e = np.full((H, W), F(2.0 ** -10), F)
    out, v0, var0 = da.denoise(c, g, e, rec)
    assert not _same(var0, v0) and not _same(out, want)
    again, _, handed = da.denoise(c, g, None, None, var0=var0)
    assert handed is var0 and _same(again, out)
