"""The facts the bounce loop's thin-lane regions rest on (csrc/pt_device.hpp: cuboid_normal's selected scale, the wave-uniform gates
around Beer's law), without a GPU: csrc/pt_math.hpp's own sequences are compiled for the HOST by hipcc with the library's arithmetic
flags (as tests/test_reference_arithmetic_abi.py compiles its probe) and compared bit for bit with the constants and with the oracle."""
import ctypes as C
import subprocess

import numpy as np
import pytest

_PROBE = r"""
#include <hip/hip_runtime.h>
// host overloads of the two bit casts the header uses (HIP declares them for the device only)
__host__ static inline float __uint_as_float(unsigned int x) { float f; __builtin_memcpy(&f, &x, 4); return f; }
__host__ static inline unsigned int __float_as_uint(float x) { unsigned int u; __builtin_memcpy(&u, &x, 4); return u; }
#define PT_DEV __host__ __device__ inline
#include "pt_math.hpp"
using namespace pt;
static float as_float(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
static uint32_t as_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
extern "C" __attribute__((visibility("default"))) uint32_t probe(int which, uint32_t x)
{
    switch (which) {
    case 0: return as_bits(f_rsqrt(as_float(x)));
    case 1: return as_bits(pt_exp<false>(as_float(x)));
    case 2: return as_bits(pt_exp<true>(as_float(x)));
    case 3: return as_bits(as_float(x) * 1.0f);
    case 4: return x == 1 ? RSQRT_1_BITS : x == 2 ? RSQRT_2_BITS : RSQRT_3_BITS;
    default: return as_bits(v_dot(V(as_float(x), 0.0f, 0.0f), V(as_float(x), 0.0f, 0.0f)));
    }
}
"""


@pytest.fixture(scope="module")
def probe(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("bounceprobe")
    src, lib = d / "probe.hip", d / "libprobe.so"
    src.write_text(_PROBE)
    flags = [f for f in pkg.native.HIPCC_FLAGS if not f.startswith("--offload-arch")]
    p = subprocess.run([pkg.native.hipcc_path(), "-x", "hip", "--cuda-host-only", *flags, "-I", pkg.native.CSRC, str(src), "-o", str(lib)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    L = C.CDLL(str(lib))
    L.probe.argtypes = [C.c_int, C.c_uint32]
    L.probe.restype = C.c_uint32
    return L.probe


def bits(x):
    return int(np.float32(x).view(np.uint32))


def test_rsqrt_constants_are_the_sequence(probe, oracle):
    """RSQRT_{1,2,3}_BITS = f_rsqrt(1), f_rsqrt(2), f_rsqrt(3) of the device header's sequence and of the oracle's; f_rsqrt(0) = +inf,
    the fourth value cuboid_normal selects"""
    want = oracle.rsqrt(np.array([0.0, 1.0, 2.0, 3.0], np.float32)).view(np.uint32)
    assert probe(0, bits(0.0)) == int(want[0]) == 0x7F800000
    assert probe(0, bits(-0.0)) == 0x7F800000
    for q in (1, 2, 3):
        assert probe(4, q) == probe(0, bits(float(q))) == int(want[q]), q
    assert probe(0, bits(1.0)) != bits(1.0)  # (one ulp below 1: the constant is the sequence's value, not the exact one)


def test_squared_length_of_a_face_normal_is_exact(probe):
    """n * n of a component in {-1, -0, +0, +1} is 0 or 1, and sums of at most three ones are exact: q is 0, 1, 2 or 3"""
    for x, want in ((1.0, 1.0), (-1.0, 1.0), (0.0, 0.0), (-0.0, 0.0)):
        assert probe(5, bits(x)) == bits(want)


def test_exp_of_both_zeros_is_one(probe, oracle):
    """the gate that skips Beer's law: pt_exp(+0) = pt_exp(-0) = 1.0f exactly, in both forms of the device function and in the oracle"""
    for z in (0.0, -0.0):
        assert probe(1, bits(z)) == probe(2, bits(z)) == bits(1.0)
        assert bits(oracle.exp(np.float32(z))) == bits(1.0)
    # -a * T of a zero absorbance and a finite T is a zero of either sign
    for a in (0.0, -0.0):
        for T in (1e-30, 0.5, 3.0e38):
            assert (bits(-np.float32(a) * np.float32(T)) & 0x7FFFFFFF) == 0


def test_times_one_keeps_every_bit(probe):
    """throughput * 1.0f: finite (normal, subnormal, zero of both signs), infinite and quiet-NaN values keep their bits"""
    rng = np.random.default_rng(11)
    words = list(rng.integers(0, 2 ** 32, 4000, dtype=np.uint64).astype(np.uint32))
    words += [0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC12345, 0x3F800000]
    for w in words:
        w = int(w)
        if (w & 0x7F800000) == 0x7F800000 and (w & 0x007FFFFF) and not (w & 0x00400000):
            continue  # a signalling NaN (the integrator produces none: every NaN it holds came out of an arithmetic operation)
        assert probe(3, w) == w, hex(w)
