"""The temporal stage of the preview denoiser without a GPU: its ABI (header, exports of the product and the diagnostic builds, argument
checks, Python and C++ harness) and the properties of the numpy restatement (tests/denoise_temporal_reference.py) that
tests/test_gpu_denoise_temporal.py compares the kernel with, bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_reference as dr
import denoise_temporal_reference as dt
import first_hit_cases as fh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355pt.h")
SYMBOLS = ["pt_denoise_set_temporal", "pt_denoise_history_clear", "pt_denoise_read_integrated", "pt_denoise_read_history"]
METHODS = ("SetDenoiseTemporal", "ClearDenoiseHistory", "DenoiseIntegrated", "DenoiseHistory")
H, W = 23, 40
F = np.float32


# ------------------------------------------------------------------------------------------------ ABI
def test_header_declares_the_four_calls_and_cites_the_host_code_they_serve():
    text = open(HEADER).read()
    h = r"PT_API\s+int\s+{}\s*\(\s*pt_handle\s+h\s*{}\s*\)\s*;"
    assert re.search(h.format("pt_denoise_set_temporal", r",\s*int\s+enable\s*,\s*int\s+max_history"), text)
    assert re.search(h.format("pt_denoise_history_clear", ""), text)
    assert re.search(h.format("pt_denoise_read_integrated", r",\s*float\s*\*\s*dst\s*,\s*size_t\s+\w+"), text)
    assert re.search(h.format("pt_denoise_read_history", r",\s*float\s*\*\s*image\s*,\s*void\s*\*\s*guides\s*,\s*float\s+out_B\[9\]\s*,\s*float\s+out_O\[3\]"), text)
    for name in SYMBOLS:
        comment = text[:text.index(f"PT_API int {name}(")].rsplit("/*", 1)[1]
        assert "MainWindow.cs:49-63" in comment and "ScreenEffect.cs:29-37" in comment, name


def test_header_still_compiles_as_c99_and_a_c_caller_links_the_names(tmp_path):
    p = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", HEADER], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    src = tmp_path / "show.c"
    src.write_text('#include "mi355pt.h"\n'
                   "int show(pt_handle h, float *img, void *guides)\n{\n"
                   "    float B[9], O[3];\n"
                   "    if (pt_denoise_set_temporal(h, 1, 32) != PT_OK || pt_denoise_render(h, 0) != PT_OK) return -1;\n"
                   "    if (pt_denoise_read_integrated(h, img, 0) != PT_OK) return -2;\n"
                   "    if (pt_denoise_read_history(h, img, guides, B, O) != PT_OK) return -3;\n"
                   "    return pt_denoise_history_clear(h);\n}\n")
    p = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "show.o")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_product_and_diagnostic_builds_export_the_four_symbols(pkg, native_lib):
    assert set(SYMBOLS) <= set(pkg.native.declared_symbols())
    paths = [pkg.native.LIB_PATH]
    for variant in pkg.native.VARIANTS:
        path = pkg.native.variant_path(variant)
        pkg.native.build_variant(variant)  # (rebuilt when older than the sources)
        paths.append(path)
    for path in paths:
        lib = C.CDLL(path)
        missing = [s for s in SYMBOLS if not hasattr(lib, s)]
        assert not missing, f"{path} lacks {missing}"


def test_calls_fail_loudly_without_a_handle_or_a_device(pkg, native_lib):
    N = pkg.native
    buf = (C.c_float * 64)()
    assert native_lib.pt_denoise_set_temporal(None, 1, 32) == N.PT_E_BAD_HANDLE
    assert native_lib.pt_denoise_history_clear(None) == N.PT_E_BAD_HANDLE
    assert native_lib.pt_denoise_read_integrated(None, buf, 0) == N.PT_E_BAD_HANDLE
    assert native_lib.pt_denoise_read_history(None, buf, None, buf, buf) == N.PT_E_BAD_HANDLE
    if native_lib.pt_device_count() == 0:  # no CPU fallback: without a device there is no handle to ask, and the harness says so
        with pytest.raises(N.NativeError) as e:
            fh.make_tracer(fh.BY_NAME["default_8x8"]).SetDenoiseTemporal(True)
        assert e.value.code == N.PT_E_NO_DEVICE


def test_python_and_cpp_harness(pkg):
    for method in METHODS:
        assert callable(getattr(pkg.PathTracer, method, None)), method
    host = open(os.path.join(pkg.native.HERE, "host", "pt_host.hpp")).read()
    for method in METHODS:
        assert re.search(rf"\b{method}\s*\(", host), method
    for name in SYMBOLS:
        assert f"{name}(h_" in host, name
    assert os.path.exists(pkg.native.build_host_demo())  # (compiles pt_host.hpp with the four methods)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in SYMBOLS:
        assert re.search(rf"extern int {name}\(", integration), name


# ------------------------------------------------------------------------------------------------ the restatement's own properties
def plane_guides(ids=None, normal=(0.0, 0.0, 1.0)):
    """A plane z = 0 seen head-on from z = 10: pos = (x, y, 0) / 10, t = 10 (built as test_denoise_cpu.py builds its own)."""
    g = np.zeros((H, W), dr.GUIDE_DTYPE)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    g["pos"][..., 0], g["pos"][..., 1] = xx * np.float32(0.1), yy * np.float32(0.1)
    g["normal"][:] = np.asarray(normal, np.float32)
    g["t"] = np.float32(10.0)
    g["id"] = 0 if ids is None else ids
    return g


def plane_camera(turned=False):
    """The camera that sees plane_guides: at O = ((W - 1) / 20, (H - 1) / 20, 10) looking down -z, pixel (x, y)'s centre on the plane point
    (x, y, 0) / 10.  With d = P - O: ndc = (20 d.x / W, 20 d.y / H) and depth -d.z / 10 = 1, so B = diag(20 / W, 20 / H, -1 / 10).
    turned: the same camera looking the other way (a turn of 180 degrees about y: x and z change sign)."""
    B = np.diag([20.0 / W, 20.0 / H, -0.1]).astype(F)
    if turned:
        B[0, 0], B[2, 2] = -B[0, 0], -B[2, 2]
    return B, np.array([(W - 1) / 20.0, (H - 1) / 20.0, 10.0], F)


def noise(seed=0, lo=0.2, hi=0.8):
    rng = np.random.default_rng(seed)
    c = np.ones((H, W, 4), np.float32)
    c[..., :3] = rng.uniform(lo, hi, (H, W, 3)).astype(np.float32)
    return c


def history(colour=0.25, count=8.0):
    h = np.empty((H, W, 4), F)
    h[..., :3], h[..., 3] = F(colour), F(count)
    return h


def _same(a, b):
    return a.tobytes() == b.tobytes()


def passthrough(c, n):
    out = c.copy()
    out[..., 3] = F(n)
    return out


def test_no_history_gives_the_image_and_n():
    c, g = noise(), plane_guides()
    assert _same(dt.integrate(c, 3, g, None, None, None, None), passthrough(c, 3))


def test_the_same_camera_and_guides_blend_every_pixel_towards_the_history():
    c, g = noise(1), plane_guides()
    B, O = plane_camera()
    I = dt.integrate(c, 2, g, history(0.25, 8.0), g, B, O)
    assert (I[..., 3] > 2).all()  # every hit pixel found history
    lo, hi = np.minimum(c[..., :3], F(0.25)), np.maximum(c[..., :3], F(0.25))
    assert (I[..., :3] >= lo - 1e-6).all() and (I[..., :3] <= hi + 1e-6).all()
    assert (np.abs(I[..., :3] - c[..., :3]) > np.abs(I[..., :3] - F(0.25))).mean() > 0.9  # 8 samples against 2: nearer the history
    # a pixel reprojects onto itself: away from the border the count is the history's (bilinear weights sum to 1 within rounding)
    assert np.allclose(I[1:-1, 1:-1, 3], 10.0, rtol=0, atol=1e-4)


def test_a_history_seen_by_a_camera_turned_180_degrees_is_not_found():
    c, g = noise(2), plane_guides()
    B, O = plane_camera(turned=True)
    assert _same(dt.integrate(c, 2, g, history(), g, B, O), passthrough(c, 2))


@pytest.mark.parametrize("n", [0, 1, 5])
@pytest.mark.parametrize("max_history", [1, 32])
def test_count_bounds_hold_exactly(n, max_history):
    """n <= count <= n + max_history everywhere and count == n on a miss: m' = min(m, max_history) >= 0 and the sum n + m' is monotone."""
    ids = np.zeros((H, W), np.int32)
    ids[:5] = -1
    ids[5:, 30:] = 256
    g, c = plane_guides(ids), noise(3)
    hist = history()
    hist[..., 3] = np.random.default_rng(4).uniform(0.0, 100.0, (H, W)).astype(F)
    B, O = plane_camera()
    O = O + np.array([0.03, 0.04, 0.0], F)  # a small shift: fractional bilinear weights
    I = dt.integrate(c, n, g, hist, g, B, O, max_history=max_history)
    count = I[..., 3]
    assert (count >= F(n)).all() and (count <= F(n) + F(max_history)).all()
    assert (count[ids == -1] == F(n)).all() and _same(I[ids == -1][..., :3], c[ids == -1][..., :3])
    assert (count[ids != -1] > F(n)).mean() > 0.9


def test_max_history_1_against_32():
    c, g = noise(5), plane_guides()
    B, O = plane_camera()
    hist = history(0.25, 64.0)
    I1 = dt.integrate(c, 1, g, hist, g, B, O, max_history=1)
    I32 = dt.integrate(c, 1, g, hist, g, B, O, max_history=32)
    assert (I1[..., 3] == 2.0).all() and (I32[..., 3] == 33.0).all()
    # the capped history weighs as one sample: the result stays nearer the image than with 32
    assert (np.abs(I1[..., :3] - c[..., :3]) < np.abs(I32[..., :3] - c[..., :3])).all()


def test_a_nan_normal_at_the_centre_passes_the_pixel_through():
    c, g = noise(6), plane_guides()
    gn = g.copy()
    gn["normal"][11, 20] = np.nan
    B, O = plane_camera()
    I = dt.integrate(c, 2, gn, history(), g, B, O)
    assert _same(I[11, 20], passthrough(c, 2)[11, 20])
    assert not np.isnan(I).any() and (I[11, 21, 3] > 2)


def test_a_history_pixel_of_another_id_contributes_nothing():
    c, g = noise(7), plane_guides()
    hg = g.copy()
    hg["id"][:, 20:] = 256  # the history saw another object on the right half
    hist = history(0.25, 8.0)
    hist[:, 20:, :3] = F(1000.0)
    B, O = plane_camera()
    I = dt.integrate(c, 2, g, hist, hg, B, O)
    assert (I[..., :3] < 1.0).all()               # nothing of the other object's colour anywhere
    assert _same(I[:, 21:], passthrough(c, 2)[:, 21:])  # and its pixels find no history at all
    assert (I[:, :19, 3] > 2).all()


def test_a_b_is_the_identity_for_the_cameras_of_the_cases():
    for case in fh.CASES:
        A, B, O = dt.camera(fh.inputs(case)[3])
        assert B.dtype == np.float32 and O.dtype == np.float32
        err = np.abs(A @ B.astype(np.float64) - np.eye(3)).max()
        assert err <= 1e-6, (case.name, err)
        assert _same(O, np.frombuffer(fh.inputs(case)[3], np.float32, 3, 64 + 48))


def test_a_real_camera_reprojects_a_pixel_onto_itself():
    """The blob of a case, analytic guides on the plane through the view direction's foot: fx, fy of the restatement's projection land
    within 1e-4 pixel of the pixel's own centre (the ray generator without jitter goes through (x + 0.5, y + 0.5))."""
    case = fh.BY_NAME["default_75x43_ap0"]
    A, B, O = dt.camera(fh.inputs(case)[3])
    Hh, Ww = case.height, case.width
    yy, xx = np.meshgrid(np.arange(Hh), np.arange(Ww), indexing="ij")
    ndc = np.stack([(xx + 0.5) / Ww * 2 - 1, (yy + 0.5) / Hh * 2 - 1, np.ones_like(xx, float)], -1)
    P = (O.astype(np.float64) + 7.0 * (ndc @ A.T)).astype(F)
    d = P - O
    p = d @ B.T
    fx = (p[..., 0] / p[..., 2] * 0.5 + 0.5) * Ww - 0.5
    fy = (p[..., 1] / p[..., 2] * 0.5 + 0.5) * Hh - 0.5
    assert (p[..., 2] > 0).all()
    assert np.abs(fx - xx).max() < 1e-4 and np.abs(fy - yy).max() < 1e-4
