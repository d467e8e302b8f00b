"""pt_atmosphere_set_arithmetic without a GPU: the ABI of the atmosphere's reference-arithmetic mode (header, exports, argument checks,
Python binding) and the device code itself — csrc/pt_atmosphere_reference.hpp is __host__ __device__, so it is compiled here for the
HOST with the library's flags and its cubes are compared with the oracle's witness build at base variant 951 bit for bit, and with the
reference's own cubes (tests/golden/atmo_*.npz) at 1e-4 on every texel.

Two host evaluations of the same header are checked: every texel on its own (atmo_texel_ref), and lane by lane through atmo_lane_ref,
the function atmo_precompute_reference_kernel runs per lane — canonical texels, x-mirror shortcut, both stores — so that the shortcut's
per-pair condition is tested against the oracle, which computes every texel directly."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as graft
import fixtures
import tolerances as tol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355pt.h")
LLVMPIPE = graft.load_oracle().LLVMPIPE  # (951) every one of llvmpipe's choices the oracle restates: oracle/pt_oracle.py


# ------------------------------------------------------------------------------------------------ (1) ABI
def test_header_declares_the_switch():
    text = open(HEADER).read()
    assert re.search(r"PT_API\s+int\s+pt_atmosphere_set_arithmetic\s*\(\s*pt_handle\s+h\s*,\s*int\s+mode\s*\)\s*;", text)


def test_product_and_diagnostic_builds_export_the_switch(pkg, native_lib):
    assert hasattr(C.CDLL(pkg.native.LIB_PATH), "pt_atmosphere_set_arithmetic")
    for variant in pkg.native.VARIANTS:
        path = pkg.native.variant_path(variant)
        if not os.path.exists(path):
            pkg.native.build_variant(variant)
        assert hasattr(C.CDLL(path), "pt_atmosphere_set_arithmetic"), f"{path} lacks pt_atmosphere_set_arithmetic"


def test_null_handle_is_rejected(pkg, native_lib):
    assert native_lib.pt_atmosphere_set_arithmetic(None, pkg.native.PT_ARITH_REFERENCE) == pkg.native.PT_E_BAD_HANDLE
    assert native_lib.pt_atmosphere_set_arithmetic(None, 7) == pkg.native.PT_E_BAD_HANDLE


def test_python_binding(pkg):
    assert "pt_atmosphere_set_arithmetic" in pkg.native.declared_symbols()
    assert callable(getattr(pkg.AtmosphericScatterer, "SetArithmetic", None))
    at = pkg.AtmosphericScatterer(32, pkg.camera.atmospheric_data_ubo(), pkg.camera.atmosphere_light_pos(0.5))
    at.SetArithmetic(pkg.native.PT_ARITH_REFERENCE)  # remembered on the object: no tracer attached yet
    with pytest.raises(ValueError):
        at.SetArithmetic(2)
    assert at._arithmetic == pkg.native.PT_ARITH_REFERENCE


def test_cpp_host_mirror_has_the_switch(pkg):
    text = open(os.path.join(os.path.dirname(pkg.native.CSRC), "host", "pt_host.hpp")).read()
    assert "void SetArithmetic(int mode)" in text and "pt_atmosphere_set_arithmetic(" in text


# ------------------------------------------------------------------------------------------------ the device code, host-compiled
_PROBE = r"""
#include "pt_atmosphere_reference.hpp"
using namespace pt::ref;
// ubo = InvProjection + 6 InvView (116 floats); out = float[6][S][S][4], must arrive filled with NaN: every texel has to be stored
extern "C" __attribute__((visibility("default"))) int atmo_cube(const float *ubo, const float *lightPos, float intensity, int S, int iSteps,
                                                                 int jSteps, int byLanes, float *out)
{
    if (!byLanes) {
        for (int face = 0; face < 6; face++)
            for (int y = 0; y < S; y++)
                for (int x = 0; x < S; x++) {
                    const pt::v3 c = atmo_texel_ref(ubo, ubo + 16, lightPos, intensity, S, iSteps, jSteps, face, x, y);
                    float *o = out + (((size_t)face * S + y) * S + x) * 4;
                    o[0] = c.x; o[1] = c.y; o[2] = c.z; o[3] = 1.0f;
                }
        return 0;
    }
    const size_t lanes = (size_t)S * atmo_row_lanes_ref(S);
    int stores = 0;
    for (size_t lane = 0; lane < lanes; lane++) {
        const AtmoLaneRef l = atmo_lane_ref(ubo, ubo + 16, lightPos, intensity, S, iSteps, jSteps, lane);
        for (int k = 0; k < l.n; k++) {
            if (l.texel[k] < 0 || l.texel[k] >= 6 * S * S) return -1;
            float *o = out + (size_t)l.texel[k] * 4;
            if (o[3] == 1.0f) return -2; // a texel stored twice
            o[0] = l.col[k].x; o[1] = l.col[k].y; o[2] = l.col[k].z; o[3] = 1.0f;
            stores++;
        }
    }
    return stores;
}
"""


@pytest.fixture(scope="module")
def host_cube(pkg, tmp_path_factory):
    """csrc/pt_atmosphere_reference.hpp compiled for the HOST by hipcc with the library's arithmetic flags (the recipe of
    tests/test_reference_arithmetic_abi.py's probe)."""
    d = tmp_path_factory.mktemp("atmoprobe")
    src, lib = d / "probe.hip", d / "libprobe.so"
    src.write_text(_PROBE)
    flags = [f for f in pkg.native.HIPCC_FLAGS if not f.startswith("--offload-arch")]
    p = subprocess.run([pkg.native.hipcc_path(), "-x", "hip", "--cuda-host-only", *flags, "-DPT_REFERENCE_PRIMITIVES_ONLY",
                        "-I", pkg.native.CSRC, str(src), "-o", str(lib)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    L = C.CDLL(str(lib))
    fp = C.POINTER(C.c_float)
    L.atmo_cube.argtypes = [fp, fp, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, fp]
    L.atmo_cube.restype = C.c_int

    def run(size, ubo, light_pos, intensity, isteps, jsteps, by_lanes):
        u = np.frombuffer(bytes(ubo), np.float32).copy()
        assert u.size == 116
        lp = np.ascontiguousarray(light_pos, np.float32)
        out = np.full((6, size, size, 4), np.nan, np.float32)
        rc = L.atmo_cube(u.ctypes.data_as(fp), lp.ctypes.data_as(fp), float(intensity), size, isteps, jsteps, int(by_lanes),
                         out.ctypes.data_as(fp))
        assert rc == (6 * size * size if by_lanes else 0), f"probe returned {rc}"
        return out
    return run


@pytest.fixture(scope="module")
def ref_oracle():
    import __graft_entry__ as graft
    o = graft.load_oracle().Oracle(perturb=True)
    o.set_base_variant(LLVMPIPE)
    yield o
    o.set_base_variant(0)


def _cases(pkg):
    """(name, size, ubo, light position, intensity, i steps, j steps, the reference's cube or None)"""
    out = []
    for name in fixtures.names("atmo_"):
        fx = fixtures.load(name)
        size, isteps, jsteps = (int(v) for v in fx["params"])
        out.append((name, size, fx["ubo"].tobytes(), np.asarray(fx["light_pos"], np.float32), float(fx["intensity"]), isteps, jsteps,
                    fx["expected"]))
    ubo = pkg.camera.atmospheric_data_ubo()
    off = np.array(pkg.camera.atmosphere_light_pos(0.4), np.float32)
    off[0] = 3.0e10                                                          # a sun off the plane x = 0: no pair may share a colour
    out.append(("sun_off_plane_40", 40, ubo, off, 15.0, 20, 6, None))
    out.append(("odd_33", 33, ubo, np.asarray(pkg.camera.atmosphere_light_pos(0.3), np.float32), 15.0, 50, 15, None))
    out.append(("pow2_64_low_sun", 64, ubo, np.asarray(pkg.camera.atmosphere_light_pos(0.52), np.float32), 22.0, 16, 4, None))
    out.append(("single_steps_16", 16, ubo, np.asarray(pkg.camera.atmosphere_light_pos(0.5), np.float32), 15.0, 1, 1, None))
    return out


def _assert_same_bits(got, want, what):
    same = got.view(np.uint32) == want.view(np.uint32)
    if not same.all():
        bad = ~same.all(-1)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} texels differ from the oracle (951); first at {np.argwhere(bad)[:5].tolist()}")


@pytest.fixture(scope="module")
def cubes(pkg, host_cube, ref_oracle):
    """name -> (texel by texel, lane by lane, oracle 951, the reference's cube or None)"""
    out = {}
    for name, size, ubo, lp, inten, isteps, jsteps, expected in _cases(pkg):
        out[name] = (host_cube(size, ubo, lp, inten, isteps, jsteps, False), host_cube(size, ubo, lp, inten, isteps, jsteps, True),
                     ref_oracle.atmosphere(size, ubo, lp, inten, isteps, jsteps, threads=16), expected)
    return out


NAMES = ["atmo_24_few_steps", "atmo_32_default", "atmo_48_noon", "sun_off_plane_40", "odd_33", "pow2_64_low_sun", "single_steps_16"]


def test_the_cases_cover_the_three_fixtures(cubes):
    assert sorted(cubes) == sorted(NAMES) and sorted(fixtures.names("atmo_")) == sorted(NAMES[:3])


# ------------------------------------------------------------------------------------------------ (2) bit-identical to the oracle at 951
@pytest.mark.parametrize("name", NAMES)
def test_host_compiled_cube_equals_oracle_951_bit_for_bit(cubes, name):
    texels, lanes, want, _ = cubes[name]
    assert np.isfinite(want).all() and (want[..., 3] == 1.0).all()
    assert (texels[..., 3] == 1.0).all() and (lanes[..., 3] == 1.0).all()
    _assert_same_bits(texels, want, f"{name}, every texel on its own")
    _assert_same_bits(lanes, want, f"{name}, lane by lane with the x-mirror shortcut")


def test_reference_arithmetic_is_not_the_contract(cubes, oracle):
    """(the comparison above is not vacuous: the witness build at 951 and the contract oracle disagree on most texels)"""
    fx = fixtures.load("atmo_32_default")
    size, isteps, jsteps = (int(v) for v in fx["params"])
    contract = oracle.atmosphere(size, fx["ubo"].tobytes(), fx["light_pos"], float(fx["intensity"]), isteps, jsteps)
    differ = (contract.view(np.uint32) != cubes["atmo_32_default"][0].view(np.uint32)).any(-1).mean()
    assert differ > 0.5, differ


# ------------------------------------------------------------------------------------------------ (3) within 1e-4 of the reference everywhere
@pytest.mark.parametrize("name", NAMES[:3])
def test_host_compiled_cube_within_1e4_of_the_reference_everywhere(cubes, name):
    texels, lanes, _, expected = cubes[name]
    for what, got in (("texels", texels), ("lanes", lanes)):
        err = tol.atmo_error(expected, got[..., :3])
        share = float((err < 1e-4).mean())
        print(f"\n  {name} ({what}): worst texel {err.max():.3g}, median {np.median(err):.3g}, share within 1e-4 {share:.4f} "
              f"(frozen contract mark {tol.ATMO_MARKS[name][1]})")
        assert err.max() < 1e-4 and share == 1.0, f"{name}: worst {err.max():.3g}, share {share:.4f}"
