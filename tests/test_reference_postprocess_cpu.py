"""pt_present_set_arithmetic without a GPU: the ABI of the tone map's reference-arithmetic mode (header, exports, argument checks, Python
binding, C++ mirror) and the device code itself — csrc/pt_postprocess_reference.hpp is __host__ __device__, so it is compiled here for
the HOST with the library's flags (tests/postprocess_probe.py) and compared with
  * the reference's own float colours (tests/golden/post_aces_gamma.npz `expected`) BIT FOR BIT, all 18,432 values;
  * the contract oracle on a ramp of 786,432 float bit patterns: floats within the 1e-6 of tests/test_oracle_vs_reference.py, RGBA8 within
    1 LSB everywhere and different somewhere (the switch is observable in the displayed image);
  * the anchors of the curve.
One anchor is stated as the reference has it, not as the feature request did: an input of -0.5 gives 0.99999994 (RGBA8 255), not 0 —
ACESFilm(-0.5) = 0.6125 / 0.4525 clamps to 1, and the fixture, which holds that very input, says so; the negative inputs that give 0 are
those in (-0.03 / 2.51, 0), where the numerator is negative (the fixture's -0.001)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fixtures
import postprocess_probe as probe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355pt.h")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ (1) ABI
def test_header_declares_the_switch():
    text = open(HEADER).read()
    assert re.search(r"PT_API\s+int\s+pt_present_set_arithmetic\s*\(\s*pt_handle\s+h\s*,\s*int\s+mode\s*\)\s*;", text)


def test_product_and_diagnostic_builds_export_the_switch(pkg, native_lib):
    assert hasattr(C.CDLL(pkg.native.LIB_PATH), "pt_present_set_arithmetic")
    for variant in pkg.native.VARIANTS:
        path = pkg.native.variant_path(variant)
        if not os.path.exists(path):
            pkg.native.build_variant(variant)
        assert hasattr(C.CDLL(path), "pt_present_set_arithmetic"), f"{path} lacks pt_present_set_arithmetic"


def test_null_handle_is_rejected(pkg, native_lib):
    assert native_lib.pt_present_set_arithmetic(None, pkg.native.PT_ARITH_REFERENCE) == pkg.native.PT_E_BAD_HANDLE
    assert native_lib.pt_present_set_arithmetic(None, 7) == pkg.native.PT_E_BAD_HANDLE


def test_python_binding(pkg):
    assert "pt_present_set_arithmetic" in pkg.native.declared_symbols()
    assert callable(getattr(pkg.PathTracer, "SetPresentArithmetic", None))
    t = object.__new__(pkg.PathTracer)  # (no handle, no device: a bad mode is refused before the library is called)
    for bad in (2, -1):
        with pytest.raises(ValueError):
            t.SetPresentArithmetic(bad)


def test_cpp_host_mirror_has_the_switch(pkg):
    text = open(os.path.join(os.path.dirname(pkg.native.CSRC), "host", "pt_host.hpp")).read()
    assert "void SetPresentArithmetic(int mode)" in text and "pt_present_set_arithmetic(" in text
    assert 'std::invalid_argument("PathTracer::SetPresentArithmetic: bad mode")' in text


def test_the_documents_no_longer_say_the_tone_map_stays_in_contract_arithmetic(pkg):
    for path in (HEADER, os.path.join(ROOT, "README.md"), os.path.join(pkg.native.CSRC, "pt_math_reference.hpp")):
        text = " ".join(open(path).read().split())
        assert "stays in contract arithmetic" not in text, path


# ------------------------------------------------------------------------------------------------ the device code, host-compiled
@pytest.fixture(scope="module")
def host(pkg, tmp_path_factory):
    return probe.build(pkg, tmp_path_factory.mktemp("ppprobe"))


def test_host_compiled_float_stage_equals_the_reference_bit_for_bit(host):
    fx = fixtures.load("post_aces_gamma")
    x, want = fx["image"][..., :3], fx["expected"]
    assert want.size == 96 * 64 * 3 == 18432 and (x < 0).any() and (x >= 1e6).any()
    got = host.floats(x)
    same = bits(got) == bits(want)
    assert same.all(), f"{int((~same).sum())} of {same.size} values differ from the reference; first inputs {x[~same][:5].tolist()}"


@pytest.fixture(scope="module")
def ramp_results(host, oracle):
    """(ramp image, host floats, host RGBA8, oracle floats, oracle RGBA8) — computed once"""
    img = probe.ramp()
    of, ou = oracle.postprocess(img)
    return img, host.floats(img[..., :3]), host.rgba8(img), of, ou


def test_ramp_floats_within_1e6_of_the_contract(ramp_results):
    img, hf, _, of, _ = ramp_results
    assert img.shape == (256, 1024, 4) and 0.99e-5 < img[..., :3].min() < 1.01e-5 and 63.9 < img[..., :3].max() < 64.0
    err = np.abs(hf - of).max()
    print(f"\n  ramp: largest |reference arithmetic - contract| in the float stage {err:.3g}")
    assert err <= 1e-6


def test_ramp_rgba8_within_one_lsb_of_the_contract_and_not_equal(ramp_results):
    img, _, hu, _, ou = ramp_results
    d = hu.astype(int) - ou.astype(int)
    assert (hu[..., 3] == 255).all() and np.abs(d).max() <= 1
    where = d != 0
    found = sorted(int(v) for v in bits(img)[where])
    print(f"\n  ramp: {int(where.sum())} of {d[..., :3].size} RGBA8 values differ between the arithmetics, inputs {[hex(v) for v in found]}")
    assert where.sum() >= 1, "the two arithmetics give the same RGBA8 on the whole ramp: the switch would not be observable"
    # the inputs the GPU tests tile into their smallest image
    assert found == sorted(probe.WITNESS_BITS)


def test_witness_tile_differs_from_the_contract_in_every_pixel(host, oracle):
    img = probe.witness_tile()
    d = host.rgba8(img)[..., :3].astype(int) - oracle.postprocess(img)[1][..., :3].astype(int)
    assert (np.abs(d) == 1).all()


def test_anchors(host):
    one = lambda x: (float(host.floats(np.array([x], np.float32))[0]), host.rgba8(np.array([[x, x, x, 0.25]], np.float32))[0].tolist())
    assert one(0.0) == (0.0, [0, 0, 0, 255])
    assert one(-0.001) == (0.0, [0, 0, 0, 255])                      # a negative numerator: clamped to 0
    assert one(-0.5) == (float(np.float32(0.99999994)), [255, 255, 255, 255])  # ACESFilm(-0.5) = 1.35 -> 1 (the reference's fixture holds this input)
    for x in (np.nan, np.inf, -np.inf):                              # NaN quotient -> maxNum(NaN, 0) = 0
        assert one(x) == (0.0, [0, 0, 0, 255]), x
    assert one(1e6)[1] == [255, 255, 255, 255]
    # alpha is 255 whatever the image holds
    a = host.rgba8(np.array([[0.5, 0.5, 0.5, a] for a in (0.0, 1.0, -3.0, np.nan, 7.0)], np.float32))
    assert (a[:, 3] == 255).all()


def test_the_branch_threshold_is_a_select(host):
    """LinearToInverseGamma switches at v = 0.0031308: the largest v below it takes v * 12.92 exactly, the threshold itself and the next
    float take the power branch — through the whole pass too, at the inputs whose ACESFilm value lands on either side."""
    thr = np.float32(0.0031308)
    under, over = np.nextafter(thr, np.float32(0)), np.nextafter(thr, np.float32(1))
    g = host.gamma(np.array([under, thr, over], np.float32))
    power = lambda v: 1.055 * float(v) ** (1.0 / 2.4) - 0.055
    assert g[0] == under * np.float32(12.92)
    for v, got in ((thr, g[1]), (over, g[2])):
        assert got != v * np.float32(12.92) and abs(float(got) - power(v)) < 1e-6
    # the first input (by bit pattern; ACESFilm rises there) whose v reaches the threshold
    lo, hi = int(bits(np.float32(0.001))[0]), int(bits(np.float32(0.02))[0])
    aces = lambda b: host.aces(np.array([b], np.uint32).view(np.float32))[0]
    assert aces(lo) < thr <= aces(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if aces(mid) >= thr else (mid, hi)
    x_under, x_over = np.array([lo], np.uint32).view(np.float32)[0], np.array([hi], np.uint32).view(np.float32)[0]
    v_under, v_over = aces(lo), aces(hi)
    assert v_under < thr <= v_over
    out = host.floats(np.array([x_under, x_over], np.float32))
    assert out[0] == v_under * np.float32(12.92)
    assert out[1] != v_over * np.float32(12.92) and abs(float(out[1]) - power(v_over)) < 1e-6
