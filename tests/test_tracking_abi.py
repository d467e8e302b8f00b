"""Object tracking of the temporal stage without a GPU (pt_denoise_set_object_tracking, pt_denoise_read_object_map): header, exports of
the product and the diagnostic builds, argument checks without a handle, the Python and C++ harnesses."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355pt.h")
SYMBOLS = ["pt_denoise_set_object_tracking", "pt_denoise_read_object_map"]
CITED = ("Gui.cs:154-218", ":163-168", ":170-210", ":212-216", "MainWindow.cs:58-63", "ScreenEffect.cs:29-37")


def test_header_declares_the_two_calls_and_cites_the_reference():
    text = open(HEADER).read()
    assert re.search(r"PT_API\s+int\s+pt_denoise_set_object_tracking\s*\(\s*pt_handle\s+h\s*,\s*int\s+enable\s*,\s*int\s+edit_max_history\s*\)\s*;", text)
    assert re.search(r"PT_API\s+int\s+pt_denoise_read_object_map\s*\(\s*pt_handle\s+h\s*,\s*void\s*\*\s*dst_320x32_bytes\s*,\s*int\s*\*\s*out_tracked\s*\)\s*;", text)
    assert re.search(r"enum\s*\{\s*PT_TRACK_KEEP\s*=\s*0\s*,\s*PT_TRACK_MOVED\s*=\s*1\s*,\s*PT_TRACK_DROP\s*=\s*2\s*\}\s*;", text)
    for name in SYMBOLS:
        comment = text[:text.index(f"PT_API int {name}(")].rsplit("/*", 1)[1]
        for cite in CITED:
            assert cite in comment, (name, cite)
    comment = text[:text.index("PT_API int pt_denoise_history_clear(")].rsplit("/*", 1)[1]
    assert "pt_denoise_set_object_tracking" in comment and "nvironment" in comment and "pt_set_params" in comment


def test_header_compiles_as_c99_and_a_c_caller_links_the_names(tmp_path):
    src = tmp_path / "track.c"
    src.write_text('#include "mi355pt.h"\n'
                   "int moved(pt_handle h, int id)\n{\n"
                   "    unsigned char map[(PT_MAX_SPHERES + PT_MAX_CUBOIDS) * 32];\n"
                   "    int tracked = 0, state;\n"
                   "    if (pt_denoise_set_object_tracking(h, 1, 0) != PT_OK || pt_denoise_render(h, 0) != PT_OK) return -1;\n"
                   "    if (pt_denoise_read_object_map(h, map, &tracked) != PT_OK) return -2;\n"
                   "    state = map[32 * id + 12];\n"
                   "    return tracked && state == PT_TRACK_MOVED ? PT_TRACK_KEEP : PT_TRACK_DROP;\n}\n")
    p = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "track.o")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_product_and_diagnostic_builds_export_the_two_symbols(pkg, native_lib):
    assert set(SYMBOLS) <= set(pkg.native.declared_symbols())
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
    assert native_lib.pt_denoise_set_object_tracking.argtypes == [C.c_void_p, C.c_int, C.c_int]
    assert native_lib.pt_denoise_read_object_map.argtypes == [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    buf, tracked = (C.c_ubyte * 10240)(), C.c_int(7)
    assert native_lib.pt_denoise_set_object_tracking(None, 1, 0) == N.PT_E_BAD_HANDLE
    assert native_lib.pt_denoise_read_object_map(None, buf, C.byref(tracked)) == N.PT_E_BAD_HANDLE
    assert native_lib.pt_denoise_read_object_map(None, None, None) == N.PT_E_BAD_HANDLE
    assert tracked.value == 7 and not any(buf)


def test_python_and_cpp_harness(pkg):
    assert (pkg.native.PT_TRACK_KEEP, pkg.native.PT_TRACK_MOVED, pkg.native.PT_TRACK_DROP) == (0, 1, 2)
    assert callable(getattr(pkg.PathTracer, "SetDenoiseTracking", None)) and callable(getattr(pkg.PathTracer, "DenoiseObjectMap", None))
    host = open(os.path.join(pkg.native.HERE, "host", "pt_host.hpp")).read()
    assert re.search(r"\bSetDenoiseTracking\s*\(", host) and "pt_denoise_set_object_tracking(h_" in host
    assert os.path.exists(pkg.native.build_host_demo())
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in SYMBOLS:
        assert re.search(r"\[DllImport\(Lib\)\][^\n]*\b" + name + r"\s*\(", integration), name
    assert "Gui.cs:212-216" in integration
