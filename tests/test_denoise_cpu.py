"""The preview denoiser without a GPU: its ABI (header, exports of the product and the diagnostic builds, argument checks, no CPU
fallback, Python and C++ harness) and the properties of the numpy restatement (tests/denoise_reference.py) that
tests/test_gpu_denoise.py compares the kernels with, bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_reference as dr
import first_hit_cases as fh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355pt.h")
SYMBOLS = ["pt_denoise_set_params", "pt_denoise_render", "pt_denoise_read", "pt_denoise_read_guides", "pt_denoise_device_ptr",
           "pt_denoise_present_rgba8"]
H, W = 23, 40


# ------------------------------------------------------------------------------------------------ ABI
def test_header_declares_the_six_calls_and_cites_the_host_code_they_serve():
    text = open(HEADER).read()
    h = r"PT_API\s+int\s+{}\s*\(\s*pt_handle\s+h\s*,\s*{}\s*\)\s*;"
    assert re.search(h.format("pt_denoise_set_params", r"int\s+iterations\s*,\s*float\s+sigma_color\s*,\s*float\s+sigma_plane\s*,\s*int\s+normal_log2_power"), text)
    assert re.search(h.format("pt_denoise_render", r"int\s+guide_frame_index"), text)
    assert re.search(h.format("pt_denoise_read", r"float\s*\*\s*dst\s*,\s*size_t\s+\w+"), text)
    assert re.search(h.format("pt_denoise_read_guides", r"void\s*\*\s*dst\s*,\s*size_t\s+\w+"), text)
    assert re.search(h.format("pt_denoise_device_ptr", r"void\s*\*\*\s*out\s*,\s*size_t\s*\*\s*bytes"), text)
    assert re.search(h.format("pt_denoise_present_rgba8", r"uint8_t\s*\*\s*dst\s*,\s*size_t\s+\w+"), text)
    for name in SYMBOLS:
        comment = text[:text.index(f"PT_API int {name}(")].rsplit("/*", 1)[1]
        assert "MainWindow.cs:49-63" in comment and "ScreenEffect.cs:29-37" in comment, name
    assert "pt_set_tile" in text[text.index("preview denoiser"):] and "62" in text[text.index("preview denoiser"):]  # the scope limit is stated


def test_header_still_compiles_as_c99_and_a_c_caller_links_the_names(tmp_path):
    p = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", HEADER], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    src = tmp_path / "show.c"
    src.write_text('#include "mi355pt.h"\n'
                   "int show(pt_handle h, float *img, void *guides, uint8_t *rgba8)\n{\n    void *p;\n    size_t n;\n"
                   "    if (pt_denoise_set_params(h, 5, 0.5f, 0.02f, 5) != PT_OK || pt_denoise_render(h, 0) != PT_OK) return -1;\n"
                   "    if (pt_denoise_read(h, img, 0) != PT_OK || pt_denoise_read_guides(h, guides, 0) != PT_OK) return -2;\n"
                   "    if (pt_denoise_device_ptr(h, &p, &n) != PT_OK || pt_denoise_present_rgba8(h, rgba8, 0) != PT_OK) return -3;\n"
                   "    return (int)(n / 16);\n}\n")
    p = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "show.o")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_product_and_diagnostic_builds_export_the_six_symbols(pkg, native_lib):
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
    buf = (C.c_char * 64)()
    assert native_lib.pt_denoise_set_params(None, 5, 0.5, 0.02, 5) == N.PT_E_BAD_HANDLE
    assert native_lib.pt_denoise_render(None, 0) == N.PT_E_BAD_HANDLE
    assert native_lib.pt_denoise_read(None, C.cast(buf, C.POINTER(C.c_float)), 0) == N.PT_E_BAD_HANDLE
    assert native_lib.pt_denoise_read_guides(None, buf, 0) == N.PT_E_BAD_HANDLE
    assert native_lib.pt_denoise_device_ptr(None, None, None) == N.PT_E_BAD_HANDLE
    assert native_lib.pt_denoise_present_rgba8(None, C.cast(buf, C.POINTER(C.c_uint8)), 0) == N.PT_E_BAD_HANDLE
    if native_lib.pt_device_count() == 0:  # no CPU fallback: without a device there is no handle to ask, and the harness says so
        h = C.c_void_p()
        assert native_lib.pt_create(0, 8, 8, C.byref(h)) == N.PT_E_NO_DEVICE and not h.value
        with pytest.raises(N.NativeError) as e:
            fh.make_tracer(fh.BY_NAME["default_8x8"]).Denoise(0)
        assert e.value.code == N.PT_E_NO_DEVICE


def test_python_and_cpp_harness(pkg):
    assert "pt_denoise.hip" in pkg.native.SOURCES
    for method in ("SetDenoise", "Denoise", "DenoiseGuides", "PresentDenoised"):
        assert callable(getattr(pkg.PathTracer, method, None)), method
    dt = pkg.path_tracer.GUIDE_DTYPE
    assert dt.itemsize == 32 and [dt.fields[n][1] for n in ("pos", "id", "normal", "t")] == [0, 12, 16, 28]
    assert dt == dr.GUIDE_DTYPE
    host = open(os.path.join(pkg.native.HERE, "host", "pt_host.hpp")).read()
    for method in ("SetDenoise", "Denoise", "DenoiseGuides", "PresentDenoised"):
        assert re.search(rf"\b{method}\s*\(", host), method
    demo = open(os.path.join(pkg.native.HERE, "host", "pt_host_demo.cpp")).read()
    assert re.search(r"Render\(\);.*?PresentDenoised\(\)", demo, re.S)
    assert os.path.exists(pkg.native.build_host_demo())  # (compiles the four methods and the demo's denoised present)


# ------------------------------------------------------------------------------------------------ the restatement's own properties
def plane_guides(ids=None, normal=(0.0, 0.0, 1.0)):
    """A plane z = 0 seen head-on from z = 10: pos = (x, y, 0), t = 10."""
    g = np.zeros((H, W), dr.GUIDE_DTYPE)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    g["pos"][..., 0], g["pos"][..., 1] = xx * np.float32(0.1), yy * np.float32(0.1)
    g["normal"][:] = np.asarray(normal, np.float32)
    g["t"] = np.float32(10.0)
    g["id"] = 0 if ids is None else ids
    return g


def noise(seed=0, lo=0.2, hi=0.8):
    rng = np.random.default_rng(seed)
    c = np.ones((H, W, 4), np.float32)
    c[..., :3] = rng.uniform(lo, hi, (H, W, 3)).astype(np.float32)
    return c


def _same(a, b):
    return a.tobytes() == b.tobytes()


def test_zero_iterations_is_the_identity():
    c = noise()
    assert _same(dr.denoise(c, plane_guides(), dr.Params(iterations=0)), c)


def test_an_all_miss_image_is_the_identity():
    g = np.zeros((H, W), dr.GUIDE_DTYPE)
    g["id"], g["t"] = -1, np.inf
    c = noise(1)
    assert _same(dr.denoise(c, g), c)


def test_no_bleed_across_an_id_edge():
    """Two ids side by side, colours exactly 0 and 1: within an id every tap has the centre's colour, so S and W are the same sum (or S is
    a sum of zeros) and the quotient is exactly 1 (or 0)."""
    ids = np.zeros((H, W), np.int32)
    ids[:, W // 2:] = 256
    c = np.ones((H, W, 4), np.float32)
    c[:, :W // 2, :3] = 0.0
    out = dr.denoise(c, plane_guides(ids))
    assert _same(out, c)


def test_a_nan_normal_at_the_centre_passes_the_pixel_through():
    g = plane_guides()
    g["normal"][11, 20] = np.nan  # (a cuboid's edge: compute.glsl:322-332 normalises a zero vector there)
    c = noise(2)
    one = dr.atrous_pass(c, g, 0, dr.Params())
    assert _same(one[11, 20], c[11, 20])
    assert not np.isnan(one).any()  # ... and as a tap of its neighbours it weighs 0
    assert (one[11, 21, :3] != c[11, 21, :3]).all()
    assert _same(dr.denoise(c, g)[11, 20], c[11, 20])


def test_variance_of_iid_noise_on_a_plane_falls_with_every_pass():
    c = noise(3, 0.4, 0.6)  # (within sigma_color of each other on the u scale: the colour weight stays open)
    g = plane_guides()
    p = dr.Params(iterations=5)
    var = [float(c[..., :3].astype(np.float64).var())]
    out = c
    for i in range(p.iterations):
        out = dr.atrous_pass(out, g, i, p)
        var.append(float(out[..., :3].astype(np.float64).var()))
    print("variance per pass:", ["%.3g" % v for v in var])
    assert all(b < a for a, b in zip(var, var[1:])), var
    assert _same(out, dr.denoise(c, g, p))


def test_inv_sigma_is_the_binary32_quotient():
    for i in range(7):
        v = dr.inv_sigma(0.5, i)
        assert v.dtype == np.float32 and float(v) == 2.0 ** (i + 1)
    assert dr.inv_sigma(0.3, 2) == np.float32(1.0) / (np.float32(0.3) * np.float32(0.25))
