"""pt_set_arithmetic without a GPU: the ABI of the reference-arithmetic mode (header, exports, argument checks, Python binding) and the
scalar primitives of csrc/pt_math_reference.hpp, host-compiled and compared bit for bit with the oracle's restatement of llvmpipe's
built-ins (oracle/pt_oracle_llvmpipe.h, witness build: pto_llvmpipe_like) and with numpy's correctly rounded 1 / x, sqrt and 1 / sqrt."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355pt.h")
N = 65536


def test_header_declares_the_mode():
    text = open(HEADER).read()
    assert re.search(r"PT_API\s+int\s+pt_set_arithmetic\s*\(\s*pt_handle\s+h\s*,\s*int\s+mode\s*\)\s*;", text)
    assert re.search(r"PT_ARITH_CONTRACT\s*=\s*0", text) and re.search(r"PT_ARITH_REFERENCE\s*=\s*1", text)


def test_product_and_diagnostic_builds_export_pt_set_arithmetic(pkg, native_lib):
    assert hasattr(C.CDLL(pkg.native.LIB_PATH), "pt_set_arithmetic")
    for variant in pkg.native.VARIANTS:
        path = pkg.native.variant_path(variant)
        if not os.path.exists(path):
            pkg.native.build_variant(variant)
        assert hasattr(C.CDLL(path), "pt_set_arithmetic"), f"{path} lacks pt_set_arithmetic"


def test_set_arithmetic_rejects_a_null_handle(pkg, native_lib):
    assert native_lib.pt_set_arithmetic(None, pkg.native.PT_ARITH_REFERENCE) == pkg.native.PT_E_BAD_HANDLE
    assert native_lib.pt_set_arithmetic(None, 7) == pkg.native.PT_E_BAD_HANDLE


def test_python_binding(pkg):
    assert (pkg.native.PT_ARITH_CONTRACT, pkg.native.PT_ARITH_REFERENCE) == (0, 1)
    assert callable(getattr(pkg.PathTracer, "SetArithmetic", None))
    assert "pt_integrate_reference.hip" in pkg.native.SOURCES


# ------------------------------------------------------------------------------------------------ the primitives, host-compiled
_PROBE = r"""
#include "pt_math_reference.hpp"
using namespace pt::ref;
extern "C" __attribute__((visibility("default"))) int probe(int which, const float *x, const float *y, int n, float *out)
{
    for (int i = 0; i < n; i++) {
        switch (which) {
        case 0: out[i] = ll_sin(x[i]); break;
        case 1: out[i] = ll_cos(x[i]); break;
        case 2: out[i] = ll_exp(x[i]); break;
        case 3: out[i] = ll_pow(x[i], y[i]); break;
        case 4: out[i] = ll_exp2(x[i]); break;
        case 5: out[i] = ll_log2(x[i]); break;
        case 6: out[i] = r_rcp(x[i]); break;
        case 7: out[i] = r_sqrt(x[i]); break;
        case 8: out[i] = r_rsqrt(x[i]); break;
        case 9: out[i] = r_pow5(x[i]); break;
        default: return -1;
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def probe(pkg, tmp_path_factory):
    """pt_math_reference.hpp's primitives compiled for the HOST by hipcc with the library's arithmetic flags."""
    d = tmp_path_factory.mktemp("refprobe")
    src, lib = d / "probe.hip", d / "libprobe.so"
    src.write_text(_PROBE)
    flags = [f for f in pkg.native.HIPCC_FLAGS if not f.startswith("--offload-arch")]
    p = subprocess.run([pkg.native.hipcc_path(), "-x", "hip", "--cuda-host-only", *flags, "-DPT_REFERENCE_PRIMITIVES_ONLY",
                        "-I", pkg.native.CSRC, str(src), "-o", str(lib)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    L = C.CDLL(str(lib))
    fp = C.POINTER(C.c_float)
    L.probe.argtypes = [C.c_int, fp, fp, C.c_int, fp]
    L.probe.restype = C.c_int

    def run(which, x, y=None):
        x = np.ascontiguousarray(x, np.float32)
        y = np.ascontiguousarray(x if y is None else y, np.float32)
        out = np.empty_like(x)
        assert L.probe(which, x.ctypes.data_as(fp), y.ctypes.data_as(fp), x.size, out.ctypes.data_as(fp)) == 0
        return out
    return run


@pytest.fixture(scope="module")
def llvmpipe_like():
    """The oracle's restatement of llvmpipe's built-ins (witness build)."""
    import __graft_entry__ as graft
    o = graft.load_oracle().Oracle(perturb=True)
    fp = C.POINTER(C.c_float)
    o.lib.pto_llvmpipe_like.argtypes = [C.c_int, fp, fp, C.c_int, fp]
    o.lib.pto_llvmpipe_like.restype = C.c_int

    def run(which, x, y=None):
        x = np.ascontiguousarray(x, np.float32)
        y = np.ascontiguousarray(x if y is None else y, np.float32)
        out = np.empty_like(x)
        assert o.lib.pto_llvmpipe_like(which, x.ctypes.data_as(fp), y.ctypes.data_as(fp), x.size, out.ctypes.data_as(fp)) == 0
        return out
    return run


def _same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _args():
    rng = np.random.default_rng(951)
    u = lambda lo, hi: rng.uniform(lo, hi, N).astype(np.float32)  # noqa: E731
    angles = np.concatenate([u(0.0, 2.0 * np.pi)[: N // 2], u(-12.6, 12.6)[: N // 2]])          # the integrator passes [0, 2 pi]
    positive = rng.integers(0, 0x7F800000, N, dtype=np.uint32).view(np.float32).copy()           # every binade, denormals included
    positive[:4] = [0.0, np.inf, 1.0, np.float32(1e-45)]
    bases = u(-0.25, 2.0)
    bases[:4] = [0.0, -0.0, np.nan, 1.0]
    return {"sin": (0, angles), "cos": (1, angles), "exp": (2, u(-104.0, 90.0)), "exp2": (4, u(-140.0, 140.0)), "log2": (5, positive),
            "pow": (3, bases, np.full(N, 5.0, np.float32)), "positive": positive}


@pytest.mark.parametrize("name", ["sin", "cos", "exp", "pow", "exp2", "log2"])
def test_llvmpipe_builtins_bit_identical_to_the_oracle(probe, llvmpipe_like, name):
    which, *xy = _args()[name]
    got, want = probe(which, *xy), llvmpipe_like(which, *xy)
    same = _same_bits(got, want)
    assert same.all(), f"{name}: {int((~same).sum())} of {N} differ, first at x = {xy[0][~same][:4]}"


def test_pow5_is_llvmpipes_pow(probe, llvmpipe_like):
    x = _args()["pow"][1]
    assert _same_bits(probe(9, x), llvmpipe_like(3, x, np.full(N, 5.0, np.float32))).all()


def test_correctly_rounded_rcp_sqrt_rsqrt(probe):
    x = _args()["positive"]
    signed = np.where(np.arange(N) % 2 == 0, x, -x).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        assert _same_bits(probe(6, signed), np.float32(1.0) / signed).all()                           # 1 / x
        assert _same_bits(probe(7, x), np.sqrt(x)).all()                                              # sqrt
        assert _same_bits(probe(8, x), np.float32(1.0) / np.sqrt(x)).all()                            # inversesqrt: 1 / sqrt, two roundings
