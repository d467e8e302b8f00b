"""The temporal moments of the preview denoiser without a GPU (pt_denoise_set_moments, pt_denoise_read_noise, pt_denoise_noise_level): the
ABI (header, exports of the product and the diagnostic builds, argument checks without a handle, Python and C++ harness) and the
properties of the numpy restatement (tests/denoise_moments_reference.py) that tests/test_gpu_denoise_moments.py compares the kernels
with, bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_moments_reference as dm
import denoise_reference as dr
import denoise_variance_reference as dv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355pt.h")
SYMBOLS = ["pt_denoise_set_moments", "pt_denoise_read_noise", "pt_denoise_noise_level"]
METHODS = ["SetDenoiseMoments", "DenoiseNoise", "DenoiseNoiseLevel"]
H, W = 23, 40
F = np.float32


# ------------------------------------------------------------------------------------------------ ABI
def test_header_declares_the_three_calls_and_cites_the_host_code_they_serve():
    text = open(HEADER).read()
    h = r"PT_API\s+int\s+{}\s*\(\s*pt_handle\s+h\s*,\s*{}\s*\)\s*;"
    assert re.search(h.format("pt_denoise_set_moments", r"int\s+enable\s*,\s*int\s+prior_samples"), text)
    assert re.search(h.format("pt_denoise_read_noise", r"float\s*\*\s*dst\s*,\s*size_t\s+row_pitch_bytes"), text)
    assert re.search(h.format("pt_denoise_noise_level", r"float\s*\*\s*out_mean_variance\s*,\s*int\s*\*\s*out_observations\s*,\s*int\s*\*\s*out_hit_pixels"), text)
    for name in SYMBOLS:
        comment = text[:text.index(f"PT_API int {name}(")].rsplit("/*", 1)[1]
        assert "MainWindow.cs:49-63" in comment and "ScreenEffect.cs:29-37" in comment, name


def test_header_compiles_as_c99_and_a_c_caller_links_the_names(tmp_path):
    src = tmp_path / "moments.c"
    src.write_text('#include "mi355pt.h"\n'
                   "int converged(pt_handle h, float *map, float threshold)\n{\n"
                   "    float mean;\n    int k, hit;\n"
                   "    if (pt_denoise_set_moments(h, 1, 32) != PT_OK || pt_denoise_render(h, 0) != PT_OK) return -1;\n"
                   "    if (pt_denoise_read_noise(h, map, 0) != PT_OK) return -2;\n"
                   "    if (pt_denoise_noise_level(h, &mean, &k, &hit) != PT_OK) return -3;\n"
                   "    return k >= 2 && hit > 0 && mean < threshold;\n}\n")
    p = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "moments.o")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_product_and_diagnostic_builds_export_the_three_symbols(pkg, native_lib):
    assert set(SYMBOLS) <= set(pkg.native.declared_symbols())
    assert "pt_denoise_moments.hip" in pkg.native.SOURCES
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
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    assert native_lib.pt_denoise_set_moments.argtypes == [C.c_void_p, C.c_int, C.c_int]
    assert native_lib.pt_denoise_read_noise.argtypes == [C.c_void_p, fp, C.c_size_t]
    assert native_lib.pt_denoise_noise_level.argtypes == [C.c_void_p, fp, ip, ip]
    buf = (C.c_float * 16)()
    assert native_lib.pt_denoise_set_moments(None, 1, 32) == N.PT_E_BAD_HANDLE
    assert native_lib.pt_denoise_read_noise(None, buf, 0) == N.PT_E_BAD_HANDLE
    assert native_lib.pt_denoise_noise_level(None, None, None, None) == N.PT_E_BAD_HANDLE


def test_python_and_cpp_harness(pkg):
    host = open(os.path.join(pkg.native.HERE, "host", "pt_host.hpp")).read()
    for method in METHODS:
        assert callable(getattr(pkg.PathTracer, method, None)), method
        assert re.search(rf"\b{method}\s*\(", host), method
    assert os.path.exists(pkg.native.build_host_demo())  # (compiles the three methods)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in SYMBOLS:
        assert re.search(r"\[DllImport\(Lib\)\][^\n]*\b" + name + r"\s*\(", integration), name


# ------------------------------------------------------------------------------------------------ the restatement's own properties
def plane_guides(ids=None, shape=(H, W)):
    """A plane z = 0 seen head-on from z = 10 (as in test_denoise_variance_cpu.py)."""
    g = np.zeros(shape, dr.GUIDE_DTYPE)
    yy, xx = np.meshgrid(np.arange(shape[0], dtype=F), np.arange(shape[1], dtype=F), indexing="ij")
    g["pos"][..., 0], g["pos"][..., 1] = xx * F(0.1), yy * F(0.1)
    g["normal"][:] = np.asarray((0.0, 0.0, 1.0), F)
    g["t"] = F(10.0)
    g["id"] = 0 if ids is None else ids
    return g


def grey(x):
    """(H, W) -> an RGBA image with r = g = b = x, alpha 1"""
    c = np.ones(x.shape + (4,), F)
    c[..., :3] = x[..., None].astype(F)
    return c


def uniform_image(seed=0, lo=0.2, hi=0.8):
    return grey(np.random.default_rng(seed).uniform(lo, hi, (H, W)))


def look_at(images):
    """images: [(n, colour)] in order -> the moment set after looking at each"""
    ms = dm.MomentSet()
    for n, c in images:
        ms = dm.observe(ms, c, n)
    return ms


def _same(a, b):
    return a.tobytes() == b.tobytes()


def test_with_fewer_than_two_observations_var_0_is_v0_and_the_filter_is_the_variance_mode():
    g = plane_guides()
    c = uniform_image()
    want, want_v0 = dv.denoise(c, g)
    for ms, n in ((dm.MomentSet(), 0), (look_at([(1, c)]), 1)):
        assert ms.K == (1 if n else 0)
        out, v0, vm, var0 = dm.denoise(c, g, ms, n)
        assert _same(var0, v0) and _same(v0, want_v0) and _same(out, want)
        assert vm.dtype == np.float32 and not vm.any()


def test_a_repeated_look_at_the_same_n_changes_nothing():
    a, b = uniform_image(1), uniform_image(2)
    ms = look_at([(1, a), (3, b)])
    again = dm.observe(ms, b, 3)
    assert again is ms
    assert again.K == 2 and again.nPrev == 3
    empty = dm.observe(dm.MomentSet(), a, 0)  # n = 0: the image holds no sample
    assert empty.K == 0
    # ... and a forgotten set starts over: another epoch, another spp, a smaller n
    for kw, n in (({"epoch": 1}, 5), ({"spp": 4}, 8), ({}, 2)):
        fresh = dm.observe(ms, b, n, **kw)
        assert fresh.K == 1 and fresh.nPrev == n and not fresh.M2.any()


SIGMA, MU, FRAMES = 0.02, 0.5, 64


def sample_plane(seed):
    """FRAMES iid Gaussian luminance samples per pixel (mean MU, deviation SIGMA) and the accumulation image after n of them."""
    s = np.random.default_rng(seed).normal(MU, SIGMA, (FRAMES, H, W))
    csum = np.cumsum(s, axis=0)
    return lambda n: grey(csum[n - 1] / n)


@pytest.mark.parametrize("block", [1, 3, 4, 8])
def test_the_measured_variance_is_the_variance_of_the_mean(block):
    """K = FRAMES // block looks, block frames apart.  s2 = M2 / (K - 1) is the unbiased sample variance of the K block means, weighted:
    for Gaussian samples its relative standard deviation is sqrt(2 / (K - 1)) per pixel.  Vm = s2 / n g(l)^4, and l, the mean of n samples,
    moves g^4 by a relative 4 (SIGMA / sqrt(n)) / (1 + MU) per pixel.  Both are independent between the H W pixels, so the image mean
    has the standard error sqrt((2 / (K - 1) + (4 SIGMA / sqrt(n) / (1 + MU))^2) / (H W)) relative to the known value, the variance of the
    mean of n samples carried to u: SIGMA^2 / n / (1 + l(MU))^4."""
    image = sample_plane(7)
    K = FRAMES // block
    n = K * block
    ms = look_at([(k * block, image(k * block)) for k in range(1, K + 1)])
    assert ms.K == K and ms.nPrev == n
    ids = np.zeros((H, W), np.int32)
    vm = dm.noise(ms, image(n), ids, n).astype(np.float64)
    l_mu = float(dm.luminance(np.full((1, 3), MU, F))[0])
    known = SIGMA ** 2 / n / (1.0 + l_mu) ** 4
    se = known * np.sqrt((2.0 / (K - 1) + (4.0 * SIGMA / np.sqrt(n) / (1.0 + MU)) ** 2) / (H * W))
    print(f"block {block}: K {K}, n {n}: mean Vm {vm.mean():.6g}, known {known:.6g}, standard error {se:.3g} ({(vm.mean() - known) / se:+.2f} of them)")
    assert (vm > 0).all()
    assert abs(vm.mean() - known) <= 4.0 * se


def test_detail_inside_one_id_is_not_noise():
    """A noise-free image with a luminance step inside one id: V0 sees the step, Vm does not.  Looks at n = 1, 2, 4, 8: nf l, npf l and
    their difference are exact, so b = l and M2 stays 0 exactly.  Looks at every n up to 16: each product rounds by at most 2^-24 n l,
    so |b - l| <= 3 n 2^-24 l, every look adds at most that squared (w = 1) to M2, and Vm <= K / (K - 1) (3 n 2^-24 l)^2 / n."""
    x = np.full((H, W), 0.2, F)
    x[:, W // 2:] = 0.7
    c = grey(x)
    g = plane_guides()
    v0 = dv.estimate(c, g)
    assert v0.max() > 1e-3
    ms = look_at([(n, c) for n in (1, 2, 4, 8)])
    vm = dm.noise(ms, c, g["id"], 8)
    assert ms.K == 4 and not ms.M2.any() and not vm.any()
    out, _, _, var0 = dm.denoise(c, g, ms, 8)
    assert (var0 <= v0).all() and (var0[v0 > 0] < v0[v0 > 0]).all()
    ms = look_at([(n, c) for n in range(1, 17)])
    vm = dm.noise(ms, c, g["id"], 16)
    bound = 16 / 15 * (3 * 16 * 2.0 ** -24 * 0.7) ** 2 / 16
    print(f"every-frame looks at a still image: max Vm {vm.max():.3g} (bound {bound:.3g}), max V0 {v0.max():.3g}")
    assert vm.max() <= bound < 1e-9 * v0.max()


def _poisoned(first, second):
    """Two looks (n = 1, 2) at a uniform image whose pixel (5, 7) holds `first` then `second` in all three channels -> (Vm, V0, var_0)"""
    a, b = uniform_image(3), uniform_image(4)
    a[5, 7, :3], b[5, 7, :3] = first, second
    g = plane_guides()
    ms = look_at([(1, a), (2, b)])
    with np.errstate(all="ignore"):
        _, v0, vm, var0 = dm.denoise(b, g, ms, 2)
    return vm, v0, var0, ms


def test_non_finite_and_negative_luminance_give_what_the_definition_gives():
    near = np.zeros((H, W), bool)
    near[5 - 4:5 + 5, 7 - 4:7 + 5] = True  # (the reach of V0's window and first differences, and of Vt's window inside it)
    # NaN in a look: b, M2 and the product are NaN, and the select sends Vm to 0 — for as long as the set lives
    for first, second in ((np.nan, 0.5), (0.5, np.nan)):
        vm, v0, var0, ms = _poisoned(first, second)
        assert np.isnan(ms.M2[5, 7]) and vm[5, 7] == 0 and np.isfinite(vm).all()
        later = dm.observe(ms, uniform_image(5), 3)
        assert np.isnan(later.M2[5, 7]) and dm.noise(later, uniform_image(5), np.zeros((H, W), np.int32), 3)[5, 7] == 0
        assert (np.isnan(var0) == np.isnan(v0)).all()  # var_0 is NaN exactly where V0 is
        assert np.isfinite(var0[~near]).all() and (var0[~near] >= 0).all()
    # +inf in both looks: nf l - npf lprev = inf - inf = NaN -> Vm = 0
    vm, v0, var0, ms = _poisoned(np.inf, np.inf)
    assert np.isnan(ms.M2[5, 7]) and vm[5, 7] == 0
    # +inf, then a finite value: b = -inf, M2 = (-inf)(-inf) = +inf, and so is Vm; Vt and var_0 of the 3x3 cells around it are +inf
    # (or NaN where V0 is), which opens their luminance stop: 1 / (k2 inf + 1e-8) = 0
    vm, v0, var0, ms = _poisoned(np.inf, 0.5)
    assert ms.M2[5, 7] == np.inf and vm[5, 7] == np.inf and np.isfinite(np.delete(vm.ravel(), 5 * W + 7)).all()
    ring = var0[4:7, 6:9]
    assert (np.isposinf(ring) | np.isnan(v0[4:7, 6:9])).all()
    assert np.isfinite(var0[~near]).all() and (var0[~near] >= 0).all()
    # -inf, then a finite value: b = +inf, M2 = (+inf)(+inf) = +inf likewise
    vm, _, _, ms = _poisoned(-np.inf, 0.5)
    assert ms.M2[5, 7] == np.inf and vm[5, 7] == np.inf
    # negative luminance is arithmetic like any other: l1 = l(-0.5), l2 = l(-0.25): b = 2 l2 - l1, M2 = (b - l1)(b - l2),
    # Vm = (M2 / 1 / 2) g^4 with g = 1 / (1 + l2) — finite and > 0
    vm, v0, var0, ms = _poisoned(-0.5, -0.25)
    l1, l2 = (dm.luminance(np.full((1, 3), v, F))[0] for v in (-0.5, -0.25))
    b = (F(2.0) * l2 - F(1.0) * l1) / F(1.0)
    m2 = F(0.0) + (F(1.0) * (b - l1)) * (b - l2)
    gg = F(1.0) / (F(1.0) + l2)
    want = (((m2 / F(1.0)) / F(2.0)) * (gg * gg)) * (gg * gg)
    assert ms.M2[5, 7] == m2 and vm[5, 7] == want and want > 0 and np.isfinite(want)
    assert np.isfinite(var0).all() and (var0 >= 0).all()
    # l = -1: g = 1 / 0 = inf; with M2 > 0 Vm = +inf, with M2 = 0 the product 0 inf is NaN and Vm = 0
    x = F(-1.0) / dm.luminance(np.ones((1, 3), F))[0]  # (the grey level whose luminance is -1, if the quotient lands on it)
    if dm.luminance(np.full((1, 3), x, F))[0] == F(-1.0):
        vm, _, _, _ = _poisoned(0.5, x)
        assert vm[5, 7] == np.inf
        vm, _, _, ms = _poisoned(x, x)
        assert vm[5, 7] == 0


def test_a_miss_has_no_noise_and_keeps_v0():
    ids = np.zeros((H, W), np.int32)
    ids[:, :5] = -1
    ids[:, 30:] = 256
    g = plane_guides(ids)
    a, b, c = uniform_image(1), uniform_image(2), uniform_image(3)
    ms = look_at([(1, a), (2, b), (3, c)])
    out, v0, vm, var0 = dm.denoise(c, g, ms, 3)
    assert not vm[ids == -1].any() and (vm[ids != -1] > 0).all()
    assert _same(var0[ids == -1], v0[ids == -1]) and not v0[ids == -1].any()
    # Vt stays inside the id: the column left of the id edge at x = 30 averages 6 cells, not 9
    vt = dm.window_mean(vm, ids)
    y = 10
    want = F(0.0)
    for dy in (-1, 0, 1):
        for dx in (-1, 0):
            want = want + vm[y + dy, 29 + dx]
    assert vt[y, 29] == want / F(6.0)
    mean, count = dm.noise_level(vm, ids)
    assert count == int((ids >= 0).sum())
    assert abs(float(mean) - vm.astype(np.float64)[ids >= 0].mean()) <= 255 * 2.0 ** -24 * float(mean)
