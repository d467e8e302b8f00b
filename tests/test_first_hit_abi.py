"""The first-hit query without a GPU: its ABI (header, exports of the product and the diagnostic builds, argument checks, no CPU
fallback, Python and C++ harness) and the soundness of the oracle decode that tests/test_gpu_first_hit.py compares the kernel's ids
with (tests/first_hit_cases.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import first_hit_cases as fh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355pt.h")
SYMBOLS = ["pt_first_hit_render", "pt_first_hit_read", "pt_first_hit_device_ptr", "pt_pick"]


def test_header_declares_the_four_calls_and_cites_what_they_replace():
    text = open(HEADER).read()
    assert re.search(r"PT_API\s+int\s+pt_first_hit_render\s*\(\s*pt_handle\s+h\s*,\s*int\s+frame_index\s*\)\s*;", text)
    assert re.search(r"PT_API\s+int\s+pt_first_hit_read\s*\(\s*pt_handle\s+h\s*,\s*void\s*\*\s*dst\s*,\s*size_t\s+row_pitch_bytes\s*\)\s*;", text)
    assert re.search(r"PT_API\s+int\s+pt_first_hit_device_ptr\s*\(\s*pt_handle\s+h\s*,\s*void\s*\*\*\s*out\s*,\s*size_t\s*\*\s*bytes\s*\)\s*;", text)
    assert re.search(r"PT_API\s+int\s+pt_pick\s*\(\s*pt_handle\s+h\s*,\s*int\s+x\s*,\s*int\s+y\s*,\s*int\s+frame_index\s*,\s*int\s*\*\s*out_id\s*,\s*"
                     r"float\s*\*\s*out_t\s*,\s*float\s+out_origin\[3\]\s*,\s*float\s+out_dir\[3\]\s*\)\s*;", text)
    for name in SYMBOLS:  # the comment in front of each declaration names the host code it replaces
        comment = text[:text.index(f"PT_API int {name}(")].rsplit("/*", 1)[1]
        assert "Gui.cs:223-233" in comment and "MainWindow.cs:302-318" in comment, name


def test_header_still_compiles_as_c99_and_a_c_caller_links_the_names(tmp_path):
    p = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", HEADER], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    src = tmp_path / "pick.c"
    src.write_text('#include "mi355pt.h"\n'
                   "int pick(pt_handle h, int x, int y)\n{\n    int id = -1;\n    float t, o[3], d[3];\n    char rec[32];\n    void *p;\n    size_t n;\n"
                   "    if (pt_pick(h, x, y, 0, &id, &t, o, d) != PT_OK) return -2;\n"
                   "    if (pt_first_hit_render(h, 0) != PT_OK || pt_first_hit_read(h, rec, 0) != PT_OK || pt_first_hit_device_ptr(h, &p, &n) != PT_OK) return -3;\n"
                   "    return id >= PT_MAX_SPHERES ? id - PT_MAX_SPHERES : id;\n}\n")
    p = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "pick.o")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_product_and_diagnostic_builds_export_the_four_symbols(pkg, native_lib):
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


def test_calls_fail_loudly_without_a_handle_or_a_device(pkg, native_lib):
    N = pkg.native
    i, t = C.c_int(), C.c_float()
    buf = (C.c_char * 32)()
    assert native_lib.pt_first_hit_render(None, 0) == N.PT_E_BAD_HANDLE
    assert native_lib.pt_first_hit_read(None, buf, 0) == N.PT_E_BAD_HANDLE
    assert native_lib.pt_first_hit_device_ptr(None, None, None) == N.PT_E_BAD_HANDLE
    assert native_lib.pt_pick(None, 0, 0, 0, C.byref(i), C.byref(t), None, None) == N.PT_E_BAD_HANDLE
    if native_lib.pt_device_count() == 0:  # no CPU fallback: without a device there is no handle to ask, and the harness says so
        h = C.c_void_p()
        assert native_lib.pt_create(0, 8, 8, C.byref(h)) == N.PT_E_NO_DEVICE and not h.value
        with pytest.raises(N.NativeError) as e:
            fh.make_tracer(fh.BY_NAME["default_8x8"]).FirstHit(0)
        assert e.value.code == N.PT_E_NO_DEVICE


def test_python_and_cpp_harness(pkg):
    assert "pt_first_hit.hip" in pkg.native.SOURCES
    assert callable(getattr(pkg.PathTracer, "FirstHit", None)) and callable(getattr(pkg.PathTracer, "Pick", None))
    dt = pkg.path_tracer.FIRST_HIT_DTYPE
    assert dt.itemsize == 32 and [dt.fields[n][1] for n in ("origin", "t", "dir", "id")] == [0, 12, 16, 28]
    assert (pkg.native.PT_MAX_SPHERES, pkg.native.PT_MAX_CUBOIDS) == (256, 64) == (fh.PT_MAX_SPHERES, 64)
    host = open(os.path.join(pkg.native.HERE, "host", "pt_host.hpp")).read()
    assert re.search(r"\bFirstHit\s*\(", host) and re.search(r"\bPick\s*\(", host)
    assert os.path.exists(pkg.native.build_host_demo())  # (compiles the two methods and the demo's MainWindow.RayTrace-style use)


@pytest.mark.parametrize("case", fh.CASES, ids=lambda c: c.name)
def test_oracle_decode_is_sound(oracle, case):
    """R (f + 1) is an integer to 1e-3 on every pixel of every case the GPU test uses, so rint(R (f + 1)) - 1 IS the oracle's first-hit id."""
    ids, residual = fh.oracle_first_hit(oracle, case)
    _, ns, nc, _ = fh.inputs(case)
    assert residual.max() < 1e-3, f"{case.name}: |R (f + 1) - rint| up to {residual.max():.3g}"
    valid = (ids == -1) | ((ids >= 0) & (ids < ns)) | ((ids >= fh.PT_MAX_SPHERES) & (ids < fh.PT_MAX_SPHERES + nc))
    assert valid.all()
    if case.scene == "empty":
        assert (ids == -1).all()
    else:
        assert (ids >= 0).any()


def test_the_cases_hold_what_they_are_meant_to(oracle):
    """The quirk cases really are quirk cases: the edge camera sees sphere 0 from inside, the cuboid camera sits in cuboid 6, the full UBO
    shows spheres and cuboids beyond the default scene's counts."""
    assert (fh.oracle_first_hit(oracle, fh.BY_NAME["edge_64x36"])[0] == 0).any()
    assert (fh.oracle_first_hit(oracle, fh.BY_NAME["incuboid_64x36"])[0] == fh.PT_MAX_SPHERES + 6).all()
    ids = fh.oracle_first_hit(oracle, fh.BY_NAME["full_64x36"])[0]
    assert ((ids >= 48) & (ids < 256)).any() and (ids >= fh.PT_MAX_SPHERES + 7).any()
    for name in ("default_75x43_ap0", "default_64x36_ap0_cam2"):
        assert fh.BY_NAME[name].aperture == 0.0
    b = np.frombuffer(fh.inputs(fh.BY_NAME["default_64x36_ap0_cam2"])[3], np.uint32)
    assert (b[28:31] == b[32:35]).all()  # InvView's translation column == ViewPos, bit for bit
