"""Shared by tests/test_reference_postprocess_cpu.py and tests/test_gpu_reference_postprocess.py: csrc/pt_postprocess_reference.hpp is
__host__ __device__, so it is compiled for the HOST by hipcc with the library's arithmetic flags (the recipe of the probes in
tests/test_reference_arithmetic_abi.py and tests/test_reference_atmosphere_cpu.py) — "the host" of the two test files — plus the inputs
both files use: the ramp of float bit patterns on which the two arithmetics differ in RGBA8, and its four witness inputs."""
import ctypes as C
import subprocess

import numpy as np

_PROBE = r"""
#include "pt_postprocess_reference.hpp"
using namespace pt::ref;
#define EXPORT extern "C" __attribute__((visibility("default")))
// the float stage (what the fragment shader writes), one value per input value
EXPORT void pp_floats(const float *x, size_t n, float *out) { for (size_t i = 0; i < n; i++) out[i] = postprocess_channel_ref(x[i]); }
// ACESFilm alone
EXPORT void pp_aces(const float *x, size_t n, float *out) { for (size_t i = 0; i < n; i++) out[i] = aces_film_ref(x[i]); }
// LinearToInverseGamma alone
EXPORT void pp_gamma(const float *v, size_t n, float *out) { for (size_t i = 0; i < n; i++) out[i] = linear_to_inverse_gamma_ref(v[i]); }
// the per-pixel function the kernel runs: RGBA32F -> RGBA8
EXPORT void pp_pixels(const float *rgba, size_t n, unsigned char *out)
{
    for (size_t i = 0; i < n; i++) {
        const uchar4 o = postprocess_pixel_ref(make_float4(rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2], rgba[4 * i + 3]));
        out[4 * i] = o.x; out[4 * i + 1] = o.y; out[4 * i + 2] = o.z; out[4 * i + 3] = o.w;
    }
}
"""

# the ramp: 1024 x 256 RGB values from the float bit patterns RAMP_FIRST + RAMP_STEP * i, channel fastest, then x, then y (1e-5 .. 63.94)
RAMP_W, RAMP_H, RAMP_FIRST, RAMP_STEP = 1024, 256, 0x3727C5AC, 242
# the four inputs of the ramp at which the contract's and the reference arithmetic's RGBA8 differ (by 1 LSB each)
WITNESS_BITS = (0x3CDA4EE0, 0x3E8DBD2E, 0x3FF36188, 0x4028CF42)


class HostPostprocess:
    def __init__(self, lib):
        self._lib = lib
        fp = C.POINTER(C.c_float)
        for name in ("pp_floats", "pp_aces", "pp_gamma"):
            getattr(lib, name).argtypes = [fp, C.c_size_t, fp]
            getattr(lib, name).restype = None
        lib.pp_pixels.argtypes = [fp, C.c_size_t, C.POINTER(C.c_uint8)]
        lib.pp_pixels.restype = None

    def _map(self, name, x):
        x = np.ascontiguousarray(x, np.float32)
        out = np.empty_like(x)
        fp = C.POINTER(C.c_float)
        getattr(self._lib, name)(x.ctypes.data_as(fp), x.size, out.ctypes.data_as(fp))
        return out

    def floats(self, x):
        return self._map("pp_floats", x)

    def aces(self, x):
        return self._map("pp_aces", x)

    def gamma(self, v):
        return self._map("pp_gamma", v)

    def rgba8(self, image):
        """(..., 4) float32 -> (..., 4) uint8"""
        img = np.ascontiguousarray(image, np.float32)
        assert img.shape[-1] == 4
        out = np.empty(img.shape, np.uint8)
        self._lib.pp_pixels(img.ctypes.data_as(C.POINTER(C.c_float)), img.size // 4, out.ctypes.data_as(C.POINTER(C.c_uint8)))
        return out


def build(pkg, directory):
    src, lib = directory / "probe.hip", directory / "libprobe.so"
    src.write_text(_PROBE)
    flags = [f for f in pkg.native.HIPCC_FLAGS if not f.startswith("--offload-arch")]
    p = subprocess.run([pkg.native.hipcc_path(), "-x", "hip", "--cuda-host-only", *flags, "-DPT_REFERENCE_PRIMITIVES_ONLY",
                        "-I", pkg.native.CSRC, str(src), "-o", str(lib)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    return HostPostprocess(C.CDLL(str(lib)))


def rgba(rgb):
    """(..., 3) float32 colours -> (..., 4) image with alpha 1 (what pt_write_result stores)"""
    rgb = np.asarray(rgb, np.float32)
    return np.concatenate([rgb, np.ones(rgb.shape[:-1] + (1,), np.float32)], axis=-1)


def ramp():
    """(RAMP_H, RAMP_W, 4) float32"""
    b = np.uint32(RAMP_FIRST) + np.uint32(RAMP_STEP) * np.arange(RAMP_W * RAMP_H * 3, dtype=np.uint32)
    return rgba(b.view(np.float32).reshape(RAMP_H, RAMP_W, 3))


def witness_tile():
    """(8, 8, 4) float32: the four witness inputs tiled over 8 x 8 x 3 colour values"""
    w = np.array(WITNESS_BITS, np.uint32).view(np.float32)
    return rgba(np.resize(w, 8 * 8 * 3).reshape(8, 8, 3))
