"""The two lens switches without a GPU (pt_first_hit_set_ray, pt_denoise_set_lens): header, exports of the product and the diagnostic
builds, argument checks without a handle, the Python and C++ harnesses."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355pt.h")
SYMBOLS = ["pt_first_hit_set_ray", "pt_denoise_set_lens"]


def test_header_declares_the_two_calls_and_cites_the_reference():
    text = open(HEADER).read()
    assert re.search(r"PT_API\s+int\s+pt_first_hit_set_ray\s*\(\s*pt_handle\s+h\s*,\s*int\s+mode\s*\)\s*;", text)
    assert re.search(r"PT_API\s+int\s+pt_denoise_set_lens\s*\(\s*pt_handle\s+h\s*,\s*int\s+enable\s*,\s*float\s+coc_scale\s*\)\s*;", text)
    assert re.search(r"enum\s*\{\s*PT_RAY_SAMPLE0\s*=\s*0\s*,\s*PT_RAY_PINHOLE\s*=\s*1\s*\}\s*;", text)
    comment = text[:text.index("PT_API int pt_first_hit_set_ray(")].rsplit("/*", 1)[1]
    assert "Gui.cs:223-233" in comment and "MainWindow.cs:302-318" in comment
    comment = text[:text.index("PT_API int pt_denoise_set_lens(")].rsplit("/*", 1)[1]
    assert "MainWindow.cs:189" in comment and "ScreenEffect.cs:29-37" in comment
    assert "only sharp at aperture 0" not in text  # (true of the default switches only: the scope comments say so now)


def test_header_compiles_as_c99_and_a_c_caller_links_the_names(tmp_path):
    src = tmp_path / "lens.c"
    src.write_text('#include "mi355pt.h"\n'
                   "int lens_on(pt_handle h)\n{\n"
                   "    if (pt_first_hit_set_ray(h, PT_RAY_PINHOLE) != PT_OK) return -1;\n"
                   "    return pt_denoise_set_lens(h, 1, 1.0f) == PT_OK ? PT_RAY_SAMPLE0 : -2;\n}\n")
    p = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "lens.o")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_product_and_diagnostic_builds_export_the_two_symbols(pkg, native_lib):
    assert set(SYMBOLS) <= set(pkg.native.declared_symbols())
    paths = [pkg.native.LIB_PATH]
    for variant in pkg.native.VARIANTS:
        path = pkg.native.variant_path(variant)
        if not os.path.exists(path):
            pkg.native.build_variant(variant)
        paths.append(path)
    for path in paths:
        lib = C.CDLL(path)
        missing = [s for s in SYMBOLS if not hasattr(lib, s)]
        assert not missing, f"{path} lacks {missing}"


def test_calls_fail_loudly_without_a_handle(pkg, native_lib):
    N = pkg.native
    assert native_lib.pt_first_hit_set_ray.argtypes == [C.c_void_p, C.c_int]
    assert native_lib.pt_denoise_set_lens.argtypes == [C.c_void_p, C.c_int, C.c_float]
    assert native_lib.pt_first_hit_set_ray(None, N.PT_RAY_PINHOLE) == N.PT_E_BAD_HANDLE
    assert native_lib.pt_denoise_set_lens(None, 1, 1.0) == N.PT_E_BAD_HANDLE


def test_python_and_cpp_harness(pkg):
    assert (pkg.native.PT_RAY_SAMPLE0, pkg.native.PT_RAY_PINHOLE) == (0, 1)
    assert callable(getattr(pkg.PathTracer, "SetFirstHitRay", None)) and callable(getattr(pkg.PathTracer, "SetDenoiseLens", None))
    host = open(os.path.join(pkg.native.HERE, "host", "pt_host.hpp")).read()
    assert re.search(r"\bSetFirstHitRay\s*\(", host) and re.search(r"\bSetDenoiseLens\s*\(", host)
    assert os.path.exists(pkg.native.build_host_demo())
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in SYMBOLS:
        assert re.search(r"\[DllImport\(Lib\)\][^\n]*\b" + name + r"\s*\(", integration), name
